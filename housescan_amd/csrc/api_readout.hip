// api_readout.hip -- the C ABI's calls that bring data to the caller and leave the volume as it is: the pinned staging pair and
// its copy pool, the downloads (volume, maps, colour, the integrate's counters), the products (cloud, meshes), views and sections.
#pragma clang fp contract(off)
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <new>
#include <pthread.h>
#include <thread>
#include <vector>

#include "hsk_ctx.h"

// ---- between device memory and the caller's PAGEABLE host memory (round 5) ------------------------------------------------
// A copy into pageable memory goes through the runtime's own staging at 16-17 GB/s, and hsk_download_tsdf moved 512 MiB
// that way (31 ms; 253 ms at 1024^3), allocating and freeing its device staging inside every call.  Two pinned buffers
// that live with the context: the device fills one (a conversion kernel writing straight into the mapped buffer, or a DMA
// copy) while host threads move the other's content to where the caller wants it.
#define HSK_PIN_BYTES ((size_t)32 << 20)
int ensure_pinned(hsk_ctx* k) {
  if (k->h_pin[0]) return HSK_OK;
  // (at least one whole plane of the volume: the download and the upload move whole planes -- 4096 x 4096 voxels are 64 MiB)
  const size_t plane = (size_t)k->vp.X * k->vp.Y * 4;
  const size_t want = plane > HSK_PIN_BYTES ? plane : HSK_PIN_BYTES;
  for (int i = 0; i < 2; ++i) {
    hipError_t e = hipHostMalloc(&k->h_pin[i], want, hipHostMallocDefault);
    if (e == hipSuccess && !k->ev_pin[i]) e = hipEventCreateWithFlags(&k->ev_pin[i], hipEventDisableTiming);
    if (e != hipSuccess) {  // (nothing half-made is left behind: the next call tries again)
      for (auto& p : k->h_pin) {
        if (p) (void)hipHostFree(p);
        p = nullptr;
      }
      HIPCHK(k, e);
    }
  }
  k->pin_bytes = want;
  return HSK_OK;
}
// Host copies out of (into) the pinned buffers are shared among a few worker threads that live with the process (started
// on first use, asleep otherwise): a core moves 10-20 GB/s, the PCIe link 55.  A thread per copy cost ~20 us each to start,
// which the pieces of a pipelined copy cannot afford.
namespace {
struct CopyPool {
  std::mutex m;
  std::condition_variable cv_work;
  std::vector<std::thread> workers;
  // a call's slices carry the call's own latch: a read-out waits for ITS slices only, whoever copies them (read-outs of
  // different contexts on different threads -- concurrent rooms, a group's slabs -- used to wait on one global count)
  struct Latch { size_t left = 0; std::condition_variable cv; };
  struct Job { char* dst; const char* src; size_t len; Latch* latch; };
  std::vector<Job> jobs;
  bool stop = false;
  void done(Latch* l) {   // (under m)
    if (--l->left == 0) l->cv.notify_all();
  }
  void worker() {
    std::unique_lock<std::mutex> lk(m);
    for (;;) {
      cv_work.wait(lk, [&] { return stop || !jobs.empty(); });
      if (stop && jobs.empty()) return;
      Job j = jobs.back();
      jobs.pop_back();
      lk.unlock();
      memcpy(j.dst, j.src, j.len);
      lk.lock();
      done(j.latch);
    }
  }
  void run(void* dst, const void* src, size_t bytes) {
    const size_t slice = (size_t)2 << 20;
    if (bytes <= slice) {
      memcpy(dst, src, bytes);
      return;
    }
    Latch latch;
    std::unique_lock<std::mutex> lk(m);
    if (workers.empty()) {
      unsigned n = std::thread::hardware_concurrency();
      n = n == 0 ? 1 : (n > 8 ? 7 : (n > 1 ? n - 1 : 1));
      for (unsigned i = 0; i < n; ++i) workers.emplace_back([this] { worker(); });
    }
    size_t first_len = 0;
    for (size_t off = 0; off < bytes; off += slice) {
      const size_t len = bytes - off < slice ? bytes - off : slice;
      if (off == 0) { first_len = len; continue; }   // the caller copies the first slice itself
      jobs.push_back(Job{(char*)dst + off, (const char*)src + off, len, &latch});
      ++latch.left;
    }
    lk.unlock();
    cv_work.notify_all();
    memcpy(dst, src, first_len);
    lk.lock();
    // (the caller helps with what is left -- its own slices or another call's -- instead of sleeping)
    while (latch.left != 0 && !jobs.empty()) {
      Job j = jobs.back();
      jobs.pop_back();
      lk.unlock();
      memcpy(j.dst, j.src, j.len);
      lk.lock();
      done(j.latch);
    }
    latch.cv.wait(lk, [&] { return latch.left == 0; });
  }
  // fork(): the child inherits `workers` without the threads behind it (joining them is undefined behaviour and hung at
  // exit) and possibly a mutex some other thread held.  The pool is quiesced round the fork and the child starts empty.
  void fork_prepare() { m.lock(); }
  void fork_parent() { m.unlock(); }
  void fork_child() {
    new (&m) std::mutex();
    new (&cv_work) std::condition_variable();
    new (&workers) std::vector<std::thread>();   // (the old vector's thread objects are abandoned, never destroyed)
    new (&jobs) std::vector<Job>();
    stop = false;
  }
  CopyPool();
  ~CopyPool() {
    {
      std::lock_guard<std::mutex> lk(m);
      stop = true;
    }
    cv_work.notify_all();
    for (auto& t : workers) t.join();
  }
};
CopyPool g_copy_pool;
CopyPool::CopyPool() {
  pthread_atfork([] { g_copy_pool.fork_prepare(); }, [] { g_copy_pool.fork_parent(); }, [] { g_copy_pool.fork_child(); });
}
}  // namespace
void parallel_memcpy(void* dst, const void* src, size_t bytes) { g_copy_pool.run(dst, src, bytes); }
// The pinned pair, outbound: `bytes` for the caller's dst in pieces of `piece`.  produce(pinned buffer, off, len) enqueues what
// fills buffer i & 1 with piece i on the stream (a DMA copy, a kernel writing into the mapped buffer); the host moves piece i - 1
// out of the other buffer meanwhile.  All of it has arrived when this returns.
template <class Produce>
static int stage_out(hsk_ctx* k, void* dst, size_t bytes, size_t piece, Produce produce) {
  const size_t n = (bytes + piece - 1) / piece;
  auto len = [&](size_t i) { return bytes - i * piece < piece ? bytes - i * piece : piece; };
  for (size_t i = 0; i <= n; ++i) {
    if (i < n) {
      const int r = produce(k->h_pin[i & 1], i * piece, len(i));
      if (r != HSK_OK) return r;
      HIPCHK(k, hipEventRecord(k->ev_pin[i & 1], k->stream));
    }
    if (i > 0) {
      HIPCHK(k, hipEventSynchronize(k->ev_pin[(i - 1) & 1]));
      parallel_memcpy((char*)dst + (i - 1) * piece, k->h_pin[(i - 1) & 1], len(i - 1));
    }
  }
  return HSK_OK;
}
// `bytes` of device memory at src into the caller's dst: the DMA of piece i + 1 runs under the host's copy of piece i
int copy_out(hsk_ctx* k, void* dst, const void* src_dev, size_t bytes) {
  int r = ensure_pinned(k);
  if (r != HSK_OK) return r;
  // (pieces of about a quarter of the whole, 2 MiB at least: the DMA of one piece and the host's copy of the one before it
  // overlap only when there are several -- a 30 MB mesh as ONE piece was 0.6 ms of DMA and then 0.75 ms of host copy)
  size_t piece = ((bytes / 4) + ((size_t)1 << 21) - 1) & ~(((size_t)1 << 21) - 1);
  if (piece < ((size_t)1 << 21)) piece = (size_t)1 << 21;
  if (piece > k->pin_bytes) piece = k->pin_bytes;
  return stage_out(k, dst, bytes, piece, [&](void* pin, size_t off, size_t len) -> int {
    HIPCHK(k, hipMemcpyAsync(pin, (const char*)src_dev + off, len, hipMemcpyDeviceToHost, k->stream));
    return HSK_OK;
  });
}

extern "C" int hsk_stored_planes(const hsk_ctx* k, int* z0, int* nz) {
  if (!k) return HSK_ERR_ARG;
  if (z0) *z0 = k->vp.zs0;
  if (nz) *nz = k->vp.nzs;
  return HSK_OK;
}

extern "C" int hsk_download_tsdf(hsk_ctx* k, int16_t* out) {
  if (!k || !out) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  flush_weights(k);  // the weights of deep free space live in the summaries until read
  // the caller's array is row-major (x fastest, then y, then plane); the volume is stored in 64-B blocks: the conversion
  // kernel writes a batch of planes straight into one of the pinned buffers while the host moves the other's out
  int r = ensure_pinned(k);
  if (r != HSK_OK) return r;
  const size_t plane_bytes = (size_t)k->vp.X * k->vp.Y * 4;
  if (plane_bytes > k->pin_bytes) return fail(k, HSK_ERR_ARG, "hsk_download_tsdf: a plane of this volume exceeds the staging buffer");
  const int batch = (int)(k->pin_bytes / plane_bytes) < k->vp.nzs ? (int)(k->pin_bytes / plane_bytes) : k->vp.nzs;
  r = stage_out(k, out, (size_t)k->vp.nzs * plane_bytes, (size_t)batch * plane_bytes, [&](void* pin, size_t off, size_t len) -> int {
    void* pin_dev = nullptr;
    HIPCHK(k, hipHostGetDevicePointer(&pin_dev, pin, 0));
    launch_vol_to_linear(k->stream, k->d_vol, k->vp, (int)(off / plane_bytes), (int)(len / plane_bytes), pin_dev);
    return HSK_OK;
  });
  if (r != HSK_OK) return r;
  HIPCHK(k, hipGetLastError());
  return HSK_OK;
}
// a plain copy between device memory and the caller's, complete on return
static int copy_sync(hsk_ctx* k, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  HIPCHK(k, hipMemcpyAsync(dst, src, bytes, kind, k->stream));
  HIPCHK(k, hipStreamSynchronize(k->stream));
  return HSK_OK;
}
static float* map_ptr(hsk_ctx* k, int kind, int level) {
  switch (kind) {
    case 0: return k->B().d_vcur[level];
    case 1: return k->B().d_ncur[level];
    case 2: return k->d_vmod[level];
    case 3: return k->d_nmod[level];
  }
  return nullptr;
}
extern "C" int hsk_download_map(hsk_ctx* k, int kind, int level, float* out) {
  if (!k || !out || level < 0 || level >= HSK_NLEVELS || kind < 0 || kind > 3) return HSK_ERR_ARG;
  return copy_sync(k, out, map_ptr(k, kind, level), (size_t)k->lv[level].W * k->lv[level].H * 12, hipMemcpyDeviceToHost);
}
extern "C" int hsk_upload_map(hsk_ctx* k, int kind, int level, const float* in) {
  if (!k || !in || level < 0 || level >= HSK_NLEVELS || kind < 0 || kind > 3) return HSK_ERR_ARG;
  return copy_sync(k, map_ptr(k, kind, level), in, (size_t)k->lv[level].W * k->lv[level].H * 12, hipMemcpyHostToDevice);
}
extern "C" int hsk_download_depth_level(hsk_ctx* k, int level, uint16_t* out) {
  if (!k || !out || level < 0 || level >= HSK_NLEVELS) return HSK_ERR_ARG;
  return copy_sync(k, out, k->B().d_dep[level], (size_t)k->lv[level].W * k->lv[level].H * 2, hipMemcpyDeviceToHost);
}
extern "C" int hsk_download_scaled_depth(hsk_ctx* k, float* out) {
  if (!k || !out) return HSK_ERR_ARG;
  return copy_sync(k, out, k->B().d_scaled, (size_t)k->lv[0].W * k->lv[0].H * 4, hipMemcpyDeviceToHost);
}

static int ensure_cube_table(hsk_ctx* k) {
  if (k->d_cube_tab) return HSK_OK;
  CubeTable ct;
  if (hsk_build_cube_table(&ct) != HSK_MC_MAXT) return fail(k, HSK_ERR_STATE, "marching-cubes table: a case with more triangles than the table holds");
  HIPCHK(k, hipMalloc((void**)&k->d_cube_tab, sizeof(CubeTable)));
  HIPCHK(k, hipMemcpy(k->d_cube_tab, &ct, sizeof(CubeTable), hipMemcpyHostToDevice));
  return HSK_OK;
}
static int ensure_row_tables(hsk_ctx* k) {
  if (k->d_rowcnt) return HSK_OK;
  const int nrows = k->vp.Y * (k->vp.zo1 - k->vp.zo0);  // (>= the mesh rows: one pair of buffers for every product)
  HIPCHK(k, hipMalloc((void**)&k->d_rowcnt, (size_t)nrows * 4));
  HIPCHK(k, hipMalloc((void**)&k->d_rowoff, hsk_scan_scratch_entries(nrows) * 8));
  return HSK_OK;
}
// the product buffer: grow-only, and when it has to grow a quarter more than asked (a scan grows from call to call) unless
// the caller names the size itself (hsk_prepare_readout)
int ensure_product_bytes(hsk_ctx* k, size_t want, bool headroom) {
  if (k->out_bytes >= want) return HSK_OK;
  if (headroom) want += want >> 2;
  if (k->d_out) (void)hipFree(k->d_out);
  k->d_out = nullptr;
  k->out_bytes = 0;
  HIPCHK(k, hipMalloc(&k->d_out, want));
  k->out_bytes = want;
  return HSK_OK;
}
extern "C" size_t hsk_product_capacity(const hsk_ctx* k) { return k ? k->out_bytes : 0; }
// n 64-bit words of device memory, once the stream has produced them
int read_u64(hsk_ctx* k, unsigned long long* dst, const unsigned long long* src_dev, int n) {
  HIPCHK(k, hipMemcpyAsync(dst, src_dev, (size_t)n * 8, hipMemcpyDeviceToHost, k->stream));
  HIPCHK(k, hipStreamSynchronize(k->stream));
  return HSK_OK;
}

// A product of the volume (cloud, mesh): counted row by row, the rows' offsets scanned, then written in voxel order.  The
// callers' protocol is a size query (null buffer) followed by the fill: the second call finds the counts and offsets of
// the first in place when nothing has touched the volume in between (ro_kind / ro_epoch) -- the count sweep ran twice
// per product before.  This is the one place that says whether d_rowcnt / d_rowoff (for kind 4 also the mesh-index scratch)
// hold product `kind`'s counts of the volume as it is; if not, count() enqueues the count pass, which leaves the totals
// (ro_totals: one, of the indexed mesh two) at d_totals.
template <class Count>
static int product_counts(hsk_ctx* k, int kind, const unsigned long long* d_totals, Count count) {
  int r = ensure_row_tables(k);
  if (r != HSK_OK) return r;
  // (NO flush of the deferred weights here, round 5: the products ask of a weight only whether it is zero, and a weight the
  // summaries hold ahead of the volume's copy is never that -- a block leaves "never observed" with a store of (+1, 1),
  // and every deferred state has all 16 weights >= 1 in the volume itself; the TSDF values are always current.  Only
  // hsk_download_tsdf, which hands the weights out, brings them up to date.  A host that shows a cloud after every
  // frame pays for the cloud, not for rewriting the frustum's free space.)
  if (k->ro_kind == kind && k->ro_epoch == k->vol_epoch) return HSK_OK;
  k->ro_kind = 0;
  count();
  k->ro_totals[1] = 0;
  r = read_u64(k, k->ro_totals, d_totals, kind == 4 ? 2 : 1);
  if (r != HSK_OK) return r;
  k->ro_kind = kind;
  k->ro_epoch = k->vol_epoch;
  return HSK_OK;
}
// ... and a product of one array: launch(d, nw) enqueues the count pass when d is null, else writes the first nw items at d.
// The product is written into the product buffer and reaches the caller through the pinned pair (copy_out).
template <class Launch>
static int extract_product(hsk_ctx* k, int kind, size_t elem_bytes, float* out, size_t cap, size_t* n_out, Launch launch) {
  int r = product_counts(k, kind, k->d_counter, [&]() { launch(nullptr, 0); });
  if (r != HSK_OK) return r;
  const unsigned long long total = k->ro_totals[0];
  *n_out = (size_t)total;
  if (!out || cap == 0 || total == 0) return HSK_OK;
  const size_t nw = total < cap ? (size_t)total : cap;
  r = ensure_product_bytes(k, nw * elem_bytes);
  if (r != HSK_OK) return r;
  launch((float*)k->d_out, nw);
  return copy_out(k, out, k->d_out, nw * elem_bytes);
}

// a view's small blocks: ViewCam, and 256 B behind it the counter slots, on the device; the same on the pinned host side
#define HSK_VIEW_COUNTS_AT 256
#define HSK_VIEW_COUNTS_BYTES ((size_t)HSK_VIEW_COUNT_SLOTS * 128)
#define HSK_VIEW_BLOCK_BYTES (HSK_VIEW_COUNTS_AT + HSK_VIEW_COUNTS_BYTES)
static int ensure_view(hsk_ctx* k) {
  if (k->d_view) return HSK_OK;
  void* d = nullptr;
  HIPCHK(k, hipMalloc(&d, HSK_VIEW_BLOCK_BYTES));
  hipError_t e = hipHostMalloc(&k->h_view, HSK_VIEW_BLOCK_BYTES, hipHostMallocDefault);
  if (e != hipSuccess) {
    (void)hipFree(d);
    k->h_view = nullptr;
    HIPCHK(k, e);
  }
  k->d_view = d;
  return HSK_OK;
}

extern "C" int hsk_prepare_readout(hsk_ctx* k, size_t product_bytes) {
  if (!k) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  int r = ensure_pinned(k);
  if (r == HSK_OK) r = ensure_row_tables(k);
  if (r == HSK_OK) r = ensure_cube_table(k);
  if (r == HSK_OK) r = ensure_product_bytes(k, product_bytes ? product_bytes : (size_t)48 << 20, false);
  if (r == HSK_OK) HIPCHK(k, (hipError_t)extract_warm());  // (the read-out kernels' code object: 0.7 ms of a process's first product)
  if (r == HSK_OK) r = ensure_view(k);
  if (r == HSK_OK) HIPCHK(k, (hipError_t)view_warm());
  if (r == HSK_OK) HIPCHK(k, (hipError_t)section_warm());
  if (r == HSK_OK) HIPCHK(k, (hipError_t)cover_warm());
  // (the labelling's scratch is as large as the volume itself: it is made by the first call that labels, not here)
  if (r == HSK_OK) HIPCHK(k, (hipError_t)comp_warm());
  if (r == HSK_OK) HIPCHK(k, (hipError_t)fill_warm());
  if (r == HSK_OK) HIPCHK(k, (hipError_t)diff_warm());
  if (r == HSK_OK) HIPCHK(k, (hipError_t)split_warm());
  if (r == HSK_OK) HIPCHK(k, (hipError_t)sweep_warm());
  if (r == HSK_OK) HIPCHK(k, (hipError_t)simplify_warm());
  if (r == HSK_OK) HIPCHK(k, (hipError_t)level_warm());
  if (r == HSK_OK) HIPCHK(k, (hipError_t)texture_warm());
  if (r == HSK_OK) HIPCHK(k, (hipError_t)keytex_warm());
  if (r == HSK_OK) HIPCHK(k, (hipError_t)splat_warm());
  if (r == HSK_OK) HIPCHK(k, (hipError_t)normals_warm());
  return r;
}

extern "C" int hsk_extract_cloud(hsk_ctx* k, float* xyz, size_t cap_points, size_t* n_points) {
  if (!k || !n_points) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  return extract_product(k, 1, 12, xyz, cap_points, n_points, [&](float* d, size_t nw) {
    launch_extract(k->stream, k->d_vol, k->vp, k->d_rowcnt, k->d_rowoff, k->d_counter, d, nw, k->d_flags);
  });
}

// Triangle soup (9 floats per triangle) of the TSDF zero level set, marching tetrahedra, voxel order.
extern "C" int hsk_extract_mesh(hsk_ctx* k, float* tri_xyz, size_t cap_triangles, size_t* n_triangles) {
  if (!k || !n_triangles) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  TetTable tt;
  hsk_build_tet_table(&tt);
  return extract_product(k, 2, 36, tri_xyz, cap_triangles, n_triangles, [&](float* d, size_t nw) {
    launch_extract_mesh(k->stream, k->d_vol, k->vp, tt, k->d_rowcnt, k->d_rowoff, k->d_counter, d, nw, k->d_flags);
  });
}

// The same level set by MARCHING CUBES (the form upstream's .ply export has, README.md:16-17): about half the triangles
// of the tetrahedra form.  Table generated by hsk_build_cube_table (PCL's own is not in the reference).
extern "C" int hsk_extract_mesh_cubes(hsk_ctx* k, float* tri_xyz, size_t cap_triangles, size_t* n_triangles) {
  if (!k || !n_triangles) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  {
    const int r = ensure_cube_table(k);
    if (r != HSK_OK) return r;
  }
  return extract_product(k, 3, 36, tri_xyz, cap_triangles, n_triangles, [&](float* d, size_t nw) {
    launch_extract_mesh_mc(k->stream, k->d_vol, k->vp, k->d_cube_tab, k->d_rowcnt, k->d_rowoff, k->d_counter, d, nw, k->d_flags);
  });
}

extern "C" int hsk_download_color(hsk_ctx* k, uint8_t* rgbw) {
  if (!k || !rgbw) return HSK_ERR_ARG;
  if (int rc = require_color(k)) return rc;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  HIPCHK(k, hipStreamSynchronize(k->stream));
  return copy_out(k, rgbw, k->d_color, k->color_bytes);
}

// The cloud with attributes, in two steps shared by hsk_extract_cloud_attrs and hsk_detect_planes_volume.  cloud_count: the count
// pass of hsk_extract_cloud (kind 1: whichever product asks first pays for it).  cloud_attrs_write: behind it, the first nw points
// into the product buffer as the arrays 0 xyz, 1 normals, 2 rgb of `pa` -- each present when it has a host pointer, xyz and
// normals also when `keep` asks for them on the device; the uncoloured points are counted in d_counter's second word (the totals
// are its first, and nothing else on the stream touches it between the memset here and the caller's read).
int cloud_count(hsk_ctx* k, size_t* total) {
  const int r = product_counts(k, 1, k->d_counter, [&]() {
    launch_extract(k->stream, k->d_vol, k->vp, k->d_rowcnt, k->d_rowoff, k->d_counter, nullptr, 0, k->d_flags);
  });
  if (r == HSK_OK) *total = (size_t)k->ro_totals[0];
  return r;
}
static int cloud_attrs_write(hsk_ctx* k, ProductArrays& pa, size_t nw, float* xyz, float* normals, uint8_t* rgb, bool keep) {
  const int a_xyz = pa.add(xyz, nw * 12, keep), a_nrm = pa.add(normals, nw * 12, keep), a_rgb = pa.add(rgb, nw * 3);
  const int r = pa.place(k);
  if (r != HSK_OK) return r;
  unsigned long long* d_uncol = k->d_counter + 1;
  HIPCHK(k, hipMemsetAsync(d_uncol, 0, 8, k->stream));
  launch_extract_attrs(k->stream, k->d_vol, k->d_color, k->vp, k->d_rowcnt, k->d_rowoff, pa.dev<float>(a_xyz), pa.dev<float>(a_nrm),
                       pa.dev<unsigned char>(a_rgb), nw, d_uncol, k->d_flags);
  HIPCHK(k, hipGetLastError());
  return HSK_OK;
}

extern "C" int hsk_extract_cloud_attrs(hsk_ctx* k, float* xyz, float* normals, uint8_t* rgb, size_t cap_points, size_t* n_points,
                                       size_t* n_uncolored) {
  if (!k || !n_points) return HSK_ERR_ARG;
  if (rgb && require_color(k)) return HSK_ERR_STATE;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  if (n_uncolored) *n_uncolored = 0;
  size_t total = 0;
  int r = cloud_count(k, &total);
  if (r != HSK_OK) return r;
  *n_points = total;
  if (!xyz || cap_points == 0 || total == 0) return HSK_OK;
  const size_t nw = total < cap_points ? total : cap_points;
  ProductArrays pa;
  r = cloud_attrs_write(k, pa, nw, xyz, normals, rgb, false);
  if (r != HSK_OK) return r;
  r = pa.copy_out(k);
  if (r == HSK_OK && rgb && n_uncolored) {
    unsigned long long u = 0;
    r = read_u64(k, &u, k->d_counter + 1);
    *n_uncolored = (size_t)u;
  }
  return r;
}

// all n > 0 points of the cloud cloud_count has counted, with their normals (packed triples), left in the product buffer for a
// device consumer: no copy out
int cloud_attrs_on_device(hsk_ctx* k, size_t n, const float** d_xyz, const float** d_normals) {
  ProductArrays pa;
  const int r = cloud_attrs_write(k, pa, n, nullptr, nullptr, nullptr, true);
  if (r != HSK_OK) return r;
  *d_xyz = pa.dev<float>(0);
  *d_normals = pa.dev<float>(1);
  return HSK_OK;
}

// hsk_extract_mesh_cubes' surface as an indexed mesh, welded on the device by edge identity (extract.hip: k_mesh_index_*).
// The count pass (edge bits, both row scans) is cached as kind 4; the faces' row tables are the shared d_rowcnt / d_rowoff.
extern "C" int hsk_extract_mesh_indexed(hsk_ctx* k, float* vertices, float* normals, uint8_t* rgb, size_t cap_vertices, size_t* n_vertices,
                                        int32_t* faces, size_t cap_faces, size_t* n_faces, size_t* n_uncolored) {
  if (!k || !n_vertices || !n_faces) return HSK_ERR_ARG;
  if (rgb && require_color(k)) return HSK_ERR_STATE;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  if (n_uncolored) *n_uncolored = 0;
  int r = ensure_cube_table(k);
  if (r != HSK_OK) return r;
  MeshIndexBufs mb;
  r = k->mi.grow(k, mesh_index_layout(k->vp, nullptr, nullptr));
  if (r != HSK_OK) return r;
  (void)mesh_index_layout(k->vp, k->mi.buf, &mb);
  r = product_counts(k, 4, mb.totals, [&]() {
    launch_mesh_index_count(k->stream, k->d_vol, k->vp, k->d_cube_tab, k->d_rowcnt, k->d_rowoff, mb, k->d_flags);
  });
  if (r != HSK_OK) return r;
  const size_t nv = (size_t)k->ro_totals[0], nf = (size_t)k->ro_totals[1];
  *n_vertices = nv;
  *n_faces = nf;
  if (nv > (size_t)INT32_MAX) return fail(k, HSK_ERR_STATE, "hsk_extract_mesh_indexed: more vertices than an int32 index reaches");
  const bool want_v = vertices || normals || rgb;
  if ((want_v && cap_vertices < nv) || (faces && cap_faces < nf))
    return fail(k, HSK_ERR_ARG, "hsk_extract_mesh_indexed: a capacity below the total (the arrays are written whole or not at all)");
  if (!(want_v && nv) && !(faces && nf)) return HSK_OK;
  ProductArrays pa;  // (an array of no items takes no space and is not copied)
  const int a_xyz = pa.add(vertices, nv * 12), a_nrm = pa.add(normals, nv * 12), a_rgb = pa.add(rgb, nv * 3), a_fc = pa.add(faces, nf * 12);
  r = pa.place(k);
  if (r != HSK_OK) return r;
  if (rgb) HIPCHK(k, hipMemsetAsync(mb.totals + 2, 0, 8, k->stream));
  launch_mesh_index_write(k->stream, k->d_vol, k->d_color, k->vp, k->d_cube_tab, k->d_rowcnt, k->d_rowoff, mb,
                          nv ? pa.dev<float>(a_xyz) : nullptr, nv ? pa.dev<float>(a_nrm) : nullptr, nv ? pa.dev<unsigned char>(a_rgb) : nullptr,
                          mb.totals + 2, nf ? pa.dev<int>(a_fc) : nullptr, k->d_flags);
  HIPCHK(k, hipGetLastError());
  r = pa.copy_out(k);
  if (r == HSK_OK && rgb && n_uncolored) {
    unsigned long long u = 0;
    r = read_u64(k, &u, mb.totals + 2);
    *n_uncolored = (size_t)u;
  }
  return r;
}

// ------------------------------------------------------------------------------------------------------
// scene views (include/hskinfu.h "Scene views")
// ------------------------------------------------------------------------------------------------------
extern "C" void hsk_default_view(const hsk_ctx* k, hsk_view* v) {
  if (!v) return;
  hsk_config c;
  if (k)
    c = k->cfg;
  else
    hsk_default_config(&c, 256);
  memset(v, 0, sizeof(*v));
  v->width = c.width;
  v->height = c.height;
  v->fx = c.fx;
  v->fy = c.fy;
  v->cx = c.cx;
  v->cy = c.cy;
  v->pose[0] = v->pose[5] = v->pose[10] = v->pose[15] = 1.0f;
  v->follow = 1;
  v->mode = HSK_VIEW_LAMBERT;
  v->light_in_camera = 1;
}

// what makes a section of a view, checked: the projection and the clip planes -> the kernel's block
static int section_clip(hsk_ctx* k, const hsk_section* s, SectionClip* clip) {
  if (s->projection != HSK_PROJ_PINHOLE && s->projection != HSK_PROJ_ORTHO)
    return fail(k, HSK_ERR_ARG, "hsk_render_section: unknown projection");
  if (s->n_clip < 0 || s->n_clip > HSK_MAX_CLIP) return fail(k, HSK_ERR_ARG, "hsk_render_section: n_clip must lie in 0..HSK_MAX_CLIP");
  memset(clip, 0, sizeof(*clip));
  clip->projection = s->projection;
  clip->n_clip = s->n_clip;
  for (int c = 0; c < s->n_clip; ++c) {
    const float* p = s->clip[c];
    if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(p[3])))
      return fail(k, HSK_ERR_ARG, "hsk_render_section: a clip plane has a non-finite number");
    if (p[0] == 0.0f && p[1] == 0.0f && p[2] == 0.0f) return fail(k, HSK_ERR_ARG, "hsk_render_section: a clip plane has no normal (a = b = c = 0)");
    clip->plane[c] = {p[0], p[1], p[2], p[3]};
  }
  return HSK_OK;
}

// The one path behind hsk_render_view (s null) and hsk_render_section (v = &s->view; its ray and tail, a third counter).  One
// launch behind whatever the stream holds; everything it writes is the product buffer and the view's own counters.  `who` names
// the call in the messages; the argument checks come first, the view's, then the section's, then the context's state.
static int render_images(hsk_ctx* k, const char* who, const char* slab_sentence, const hsk_view* v, const hsk_section* s, uint8_t* rgb,
                         uint16_t* depth_mm, float* vmap, float* nmap, size_t* n_hit, size_t* n_cut, size_t* n_uncolored) {
  auto bad_arg = [&](const char* what) { return fail(k, HSK_ERR_ARG, (std::string(who) + what).c_str()); };
  if (v->width < 1 || v->width > 4096 || v->height < 1 || v->height > 4096) return bad_arg(": width and height must lie in 1..4096");
  if (!(std::isfinite(v->fx) && std::isfinite(v->fy) && v->fx > 0.0f && v->fy > 0.0f)) return bad_arg(": fx and fy must be finite and positive");
  if (v->mode < HSK_VIEW_LAMBERT || v->mode > HSK_VIEW_COLOR_LIT) return bad_arg(": unknown mode");
  SectionClip clip;
  int r = s ? section_clip(k, s, &clip) : HSK_OK;
  if (r == HSK_OK) r = require_whole_volume(k, k, who, slab_sentence);
  if (r == HSK_OK && (v->mode == HSK_VIEW_COLOR || v->mode == HSK_VIEW_COLOR_LIT)) r = require_color(k);
  if (r != HSK_OK) return r;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  r = ensure_view(k);
  if (r != HSK_OK) return r;
  const size_t P = (size_t)v->width * v->height;
  ProductArrays pa;
  const int a_rgb = pa.add(rgb, P * 3), a_dep = pa.add(depth_mm, P * 2), a_v = pa.add(vmap, P * 12), a_n = pa.add(nmap, P * 12);
  r = pa.place(k);
  if (r != HSK_OK) return r;
  unsigned char* d_rgb = pa.dev<unsigned char>(a_rgb);
  unsigned short* d_dep = pa.dev<unsigned short>(a_dep);
  float *d_v = pa.dev<float>(a_v), *d_n = pa.dev<float>(a_n);
  // the camera: the tracker's own state, read by the kernel where the stream has got to (follow), or the view's block
  const ViewCam* cam = (const ViewCam*)k->d_st;
  if (!v->follow) {
    ViewCam* hc = (ViewCam*)k->h_view;   // (free: every call waits for its own result before it returns)
    pose16_to_rt(v->pose, hc->R, hc->t);
    HIPCHK(k, hipMemcpyAsync(k->d_view, hc, sizeof(ViewCam), hipMemcpyHostToDevice, k->stream));
    cam = (const ViewCam*)k->d_view;
  }
  unsigned long long* d_counts = (unsigned long long*)((char*)k->d_view + HSK_VIEW_COUNTS_AT);
  unsigned long long* h_counts = (unsigned long long*)((char*)k->h_view + HSK_VIEW_COUNTS_AT);
  HIPCHK(k, hipMemsetAsync(d_counts, 0, HSK_VIEW_COUNTS_BYTES, k->stream));
  const Intr in = {v->fx, v->fy, v->cx, v->cy};
  if (!s)
    launch_render_view(k->stream, k->d_vol, k->d_color, cam, k->vp, v->width, v->height, in, k->d_flags, v->mode, v->light,
                       v->light_in_camera, v->background, d_rgb, d_dep, d_v, d_n, d_counts);
  else
    launch_render_section(k->stream, k->d_vol, k->d_color, cam, k->vp, v->width, v->height, in, k->d_flags, v->mode, v->light,
                          v->light_in_camera, s->light_directional != 0, v->background, s->cut_rgb, clip, d_rgb, d_dep, d_v, d_n, d_counts);
  HIPCHK(k, hipGetLastError());
  HIPCHK(k, hipMemcpyAsync(h_counts, d_counts, HSK_VIEW_COUNTS_BYTES, hipMemcpyDeviceToHost, k->stream));
  r = pa.copy_out(k);
  if (r != HSK_OK) return r;
  HIPCHK(k, hipStreamSynchronize(k->stream));
  unsigned long long sum[3] = {0, 0, 0};  // hits, hits without colour, cut pixels (a section's)
  for (int i = 0; i < HSK_VIEW_COUNT_SLOTS; ++i)
    for (int c = 0; c < 3; ++c) sum[c] += h_counts[16 * i + c];
  if (n_hit) *n_hit = (size_t)sum[0];
  if (n_uncolored) *n_uncolored = (size_t)sum[1];
  if (n_cut) *n_cut = (size_t)sum[2];
  return HSK_OK;
}

extern "C" int hsk_render_view(hsk_ctx* k, const hsk_view* v, uint8_t* rgb, uint16_t* depth_mm, float* vmap, float* nmap, size_t* n_hit,
                               size_t* n_uncolored) {
  if (!k) return HSK_ERR_ARG;
  if (!v) return fail(k, HSK_ERR_ARG, "hsk_render_view: view is null");
  return render_images(k, "hsk_render_view", "it owns only its own march steps; views are not composited", v, nullptr, rgb, depth_mm, vmap,
                       nmap, n_hit, nullptr, n_uncolored);
}

// ------------------------------------------------------------------------------------------------------
// section views (include/hskinfu.h "Section views")
// ------------------------------------------------------------------------------------------------------
extern "C" void hsk_default_section(const hsk_ctx* k, hsk_section* s) {
  if (!s) return;
  memset(s, 0, sizeof(*s));
  hsk_default_view(k, &s->view);
  s->projection = HSK_PROJ_PINHOLE;
  s->cut_rgb[0] = 255;
  s->cut_rgb[1] = 96;
  s->cut_rgb[2] = 0;
}

extern "C" int hsk_render_section(hsk_ctx* k, const hsk_section* s, uint8_t* rgb, uint16_t* depth_mm, float* vmap, float* nmap,
                                  size_t* n_hit, size_t* n_cut, size_t* n_uncolored) {
  if (!k) return HSK_ERR_ARG;
  if (!s) return fail(k, HSK_ERR_ARG, "hsk_render_section: section is null");
  return render_images(k, "hsk_render_section", "it owns only its own march steps; sections of a group are not composited", &s->view, s,
                       rgb, depth_mm, vmap, nmap, n_hit, n_cut, n_uncolored);
}

// lane-blocks (4 x 1 x 4 voxels) the last integrate's classification pass handed to its per-voxel pass
static int queue_counters(hsk_ctx* k, uint64_t* n_entries, unsigned long long (*sum)(const unsigned*)) {
  if (!k || !n_entries) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  const size_t words = integrate_queue_counter_words();
  unsigned* h = (unsigned*)malloc(words * 4);
  if (!h) return fail(k, HSK_ERR_STATE, "out of host memory");
  hipError_t e = hipMemcpyAsync(h, k->d_queue, words * 4, hipMemcpyDeviceToHost, k->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(k->stream);
  const uint64_t n = e == hipSuccess ? sum(h) : 0;
  free(h);
  HIPCHK(k, e);
  *n_entries = n;
  return HSK_OK;
}
extern "C" int hsk_integrate_queue_entries(hsk_ctx* k, uint64_t* n_entries) { return queue_counters(k, n_entries, integrate_queue_entries); }
// ... and of those, the lane-blocks of the LIGHT class (free space with holes in the depth image under it: hsk_integrate_queue_entries
// counts the per-voxel class only)
extern "C" int hsk_integrate_light_entries(hsk_ctx* k, uint64_t* n_entries) {
  return queue_counters(k, n_entries, integrate_queue_light_entries);
}
extern "C" int hsk_integrate_coarse_counts(hsk_ctx* k, uint64_t counts[4]) {
  if (!k || !counts) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  const size_t n = integrate_chunk_count(k->vp);
  unsigned char* h = (unsigned char*)malloc(2 * n);
  if (!h) return fail(k, HSK_ERR_STATE, "out of host memory");
  hipError_t e = hipMemcpyAsync(h, (const char*)k->d_zint + integrate_cflag_offset_bytes(k->vp), n, hipMemcpyDeviceToHost, k->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h + n, k->d_uni + uniform_lane_bytes(k->vp), n, hipMemcpyDeviceToHost, k->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(k->stream);
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  for (size_t i = 0; i < n && e == hipSuccess; ++i) {
    if (h[i] < 3) counts[h[i]] += 1;
    if (h[n + i] != 0) counts[3] += 1;
  }
  free(h);
  HIPCHK(k, e);
  return HSK_OK;
}
