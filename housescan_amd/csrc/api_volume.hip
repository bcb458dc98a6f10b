// api_volume.hip -- the C ABI's calls that replace or serialise the volume: the uploads, hsk_fuse_volume, the volume files
// (pack, unpack, save, load, the *_info calls) and resuming a scan on a restored volume.
#pragma clang fp contract(off)
#include <new>
#include <vector>

#include "hsk_ctx.h"

// The pinned pair, inbound: the host range `from` in pieces of `piece`.  Piece *turn goes into buffer *turn & 1 once the stream's
// use of that buffer two pieces ago has ended, and consume(pinned buffer, off, len) enqueues what takes it from there (a DMA
// copy, a kernel reading the mapped buffer).  *turn counts the pieces of the whole call, over all its ranges.
template <class Consume>
static int stage_in(hsk_ctx* k, int* turn, const void* from, size_t bytes, size_t piece, Consume consume) {
  for (size_t off = 0; off < bytes; off += piece, ++*turn) {
    const size_t len = bytes - off < piece ? bytes - off : piece;
    const int b = *turn & 1;
    if (*turn >= 2) HIPCHK(k, hipEventSynchronize(k->ev_pin[b]));
    parallel_memcpy(k->h_pin[b], (const char*)from + off, len);
    const int r = consume(k->h_pin[b], off, len);
    if (r != HSK_OK) return r;
    HIPCHK(k, hipEventRecord(k->ev_pin[b], k->stream));
  }
  return HSK_OK;
}
// (hsk_ctx.h: the brick bitfield and both summary levels made again behind whatever wrote the volume)
int volume_replaced(hsk_ctx* k) {
  k->vol_epoch += 1;
  HIPCHK(k, hipMemsetAsync(k->d_flags, 0, k->flags_bytes, k->stream));
  launch_rebuild_flags(k->stream, k->d_vol, k->vp, k->d_flags);
  launch_rebuild_uniform(k->stream, k->d_vol, k->vp, k->d_uni);
  return HSK_OK;
}

int commit_volume_write(hsk_ctx* k, const std::function<void()>& launch) {
  flush_weights(k);
  launch();
  HIPCHK(k, hipGetLastError());
  const int r = volume_replaced(k);
  if (r != HSK_OK) return r;
  HIPCHK(k, hipStreamSynchronize(k->stream));
  HIPCHK(k, hipGetLastError());
  return HSK_OK;
}

extern "C" int hsk_flush_weights(hsk_ctx* k) {
  if (!k) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  flush_weights(k);
  HIPCHK(k, hipGetLastError());
  return HSK_OK;
}
extern "C" int hsk_upload_tsdf(hsk_ctx* k, const int16_t* in) {
  if (!k || !in) return HSK_ERR_ARG;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  int r = ensure_pinned(k);
  if (r != HSK_OK) return r;
  const size_t plane_bytes = (size_t)k->vp.X * k->vp.Y * 4;
  if (plane_bytes > k->pin_bytes) return fail(k, HSK_ERR_ARG, "hsk_upload_tsdf: a plane of this volume exceeds the staging buffer");
  const int batch = (int)(k->pin_bytes / plane_bytes) < k->vp.nzs ? (int)(k->pin_bytes / plane_bytes) : k->vp.nzs;
  HIPCHK(k, hipMemsetAsync(k->d_vol, 0, k->vol_bytes, k->stream));  // (the padding planes of the last block row)
  int turn = 0;  // (a piece is a batch of whole planes: the kernel reads them out of the mapped buffer)
  r = stage_in(k, &turn, in, (size_t)k->vp.nzs * plane_bytes, (size_t)batch * plane_bytes, [&](void* pin, size_t off, size_t len) -> int {
    void* pin_dev = nullptr;
    HIPCHK(k, hipHostGetDevicePointer(&pin_dev, pin, 0));
    launch_vol_from_linear(k->stream, k->d_vol, k->vp, (int)(off / plane_bytes), (int)(len / plane_bytes), pin_dev);
    return HSK_OK;
  });
  if (r == HSK_OK) r = volume_replaced(k);
  if (r != HSK_OK) return r;
  HIPCHK(k, hipStreamSynchronize(k->stream));
  return HSK_OK;
}

extern "C" int hsk_upload_color(hsk_ctx* k, const uint8_t* rgbw) {
  if (!k || !rgbw) return HSK_ERR_ARG;
  if (int rc = require_color(k)) return rc;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  HIPCHK(k, hipMemcpyAsync(k->d_color, rgbw, k->color_bytes, hipMemcpyHostToDevice, k->stream));
  k->pack.drop();  // (the volume image's pass is void)
  HIPCHK(k, hipStreamSynchronize(k->stream));
  return HSK_OK;
}

// ------------------------------------------------------------------------------------------------------
// volume fusion (include/hskinfu.h "Volume fusion")
// ------------------------------------------------------------------------------------------------------
#define HSK_FUSE_COUNTS_BYTES 64

extern "C" int hsk_fuse_volume(hsk_ctx* dst, hsk_ctx* src, const float src_to_dst[16], hsk_fuse_stats* stats) {
  if (!dst) return HSK_ERR_ARG;
  if (!src || !src_to_dst) return fail(dst, HSK_ERR_ARG, "hsk_fuse_volume: null argument");
  if (src == dst) return fail(dst, HSK_ERR_ARG, "hsk_fuse_volume: source and destination are the same context");
  float inv[16];
  if (hsk_invert_rigid(src_to_dst, inv) != HSK_OK)
    return fail(dst, HSK_ERR_ARG, "hsk_fuse_volume: src_to_dst is not rigid (last row 0 0 0 1, |R^T R - I| <= 1e-4)");
  if (memcmp(&dst->vp.tau, &src->vp.tau, sizeof(float)) != 0)
    return fail(dst, HSK_ERR_ARG, "hsk_fuse_volume: the contexts' effective truncation distances differ (stored TSDF values are in units of it)");
  if (dst->cfg.device_id != src->cfg.device_id) return fail(dst, HSK_ERR_ARG, "hsk_fuse_volume: the contexts are on different devices");
  for (hsk_ctx* c : {dst, src})
    if (int rs = require_whole_volume(c, dst, "hsk_fuse_volume")) return rs;
  for (hsk_ctx* c : {dst, src})
    if (int ri = require_idle(c, dst)) return ri;
  hsk_fuse_stats st;
  memset(&st, 0, sizeof(st));
  const int sdims[3] = {src->vp.X, src->vp.Y, src->vp.Z}, ddims[3] = {dst->vp.X, dst->vp.Y, dst->vp.Z};
  if (hsk_fuse_footprint(sdims, src->vp.size, ddims, dst->vp.size, src_to_dst, st.box) != HSK_OK)
    return fail(dst, HSK_ERR_ARG, "hsk_fuse_volume: no footprint for these volumes");
  if (st.box[1] <= st.box[0]) {  // nothing of the source's interior reaches the destination
    if (stats) *stats = st;
    return HSK_OK;
  }
  hsk_ctx* k = dst;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  // the source: read only.  The rule reads weights, so its deferred ones are written back first (which changes nothing it
  // returns); everything its stream holds must have ended before the destination's stream reads the volume
  flush_weights(src);
  HIPCHK(k, hipStreamSynchronize(src->stream));
  flush_weights(k);
  const size_t tab_bytes = fuse_table_words(src->vp) * 4;
  if (k->fuse_bytes < HSK_FUSE_COUNTS_BYTES + tab_bytes) {
    if (k->d_fuse) HIPCHK(k, hipFree(k->d_fuse));
    k->d_fuse = nullptr;
    k->fuse_bytes = 0;
    HIPCHK(k, hipMalloc(&k->d_fuse, HSK_FUSE_COUNTS_BYTES + tab_bytes));
    k->fuse_bytes = HSK_FUSE_COUNTS_BYTES + tab_bytes;
  }
  unsigned long long* d_counts = (unsigned long long*)k->d_fuse;
  unsigned* d_tab = (unsigned*)((char*)k->d_fuse + HSK_FUSE_COUNTS_BYTES);
  HIPCHK(k, hipMemsetAsync(k->d_fuse, 0, HSK_FUSE_COUNTS_BYTES + tab_bytes, k->stream));
  launch_fuse_bricks(k->stream, src->d_vol, src->vp, d_tab);
  const bool colour = k->d_color && src->d_color;
  unsigned long long chunks_total = 0;
  float A[9], b[3];
  pose16_to_rt(inv, A, b);
  launch_fuse_sweep(k->stream, src->d_vol, colour ? src->d_color : nullptr, k->d_vol, colour ? k->d_color : nullptr, src->vp, k->vp, A, b,
                    st.box, d_tab, k->color_max_w, d_counts, &chunks_total);
  HIPCHK(k, hipGetLastError());
  if (int rv = volume_replaced(k)) return rv;
  HIPCHK(k, hipGetLastError());
  unsigned long long counts[3] = {0, 0, 0};
  int r = read_u64(k, counts, d_counts, 3);
  if (r != HSK_OK) return r;
  st.n_fused = counts[0];
  st.n_colored = counts[1];
  st.chunks_swept = counts[2];
  st.chunks_total = chunks_total;
  if (stats) *stats = st;
  return HSK_OK;
}

// ------------------------------------------------------------------------------------------------------
// volume files (include/hskinfu.h "Volume files")
// ------------------------------------------------------------------------------------------------------
// the pack scratch, carved out of pack's buffer: counters (8 words for the TSDF, 8 for the colour), the class tables (zero-padded to
// the image's table length), the size / offset tables, the scan's block sums
struct PackBufs {
  size_t n_bricks, table_bytes, bytes;
  unsigned* counts;
  unsigned char *cls_t, *cls_c;
  unsigned *off_t, *off_c, *bsum;
};
static PackBufs pack_bufs(const hsk_ctx* k) {
  PackBufs b;
  b.n_bricks = pack_bricks(k->vp);
  b.table_bytes = (size_t)hskv_table_bytes(b.n_bricks);
  ProductLayout l;
  char* base = (char*)k->pack.buf;
  b.counts = (unsigned*)(base + l.take(64));
  b.cls_t = (unsigned char*)(base + l.take(b.table_bytes));
  b.cls_c = (unsigned char*)(base + l.take(b.table_bytes));
  b.off_t = (unsigned*)(base + l.take(b.n_bricks * 4));
  b.off_c = (unsigned*)(base + l.take(b.n_bricks * 4));
  b.bsum = (unsigned*)(base + l.take((pack_scan_blocks(b.n_bricks) + 1) * 4));
  b.bytes = l.bytes;
  return b;
}
static int ensure_pack(hsk_ctx* k) {
  if (k->pack.buf) return HSK_OK;
  const size_t bytes = pack_bufs(k).bytes;
  const int r = k->pack.grow(k, bytes);
  if (r != HSK_OK) return r;
  const hipError_t e = hipMemsetAsync(k->pack.buf, 0, bytes, k->stream);  // (the tables' padding stays zero from here on)
  if (e != hipSuccess) {
    (void)k->pack.release(k);
    HIPCHK(k, e);
  }
  return HSK_OK;
}
// the state every call of this section needs: a context that stores its whole volume, with no frame in flight
static int pack_state_check(hsk_ctx* k, const char* who) {
  const int r = require_whole_volume(k, k, who);
  return r != HSK_OK ? r : require_idle(k);
}
// the header fields that come from the context rather than from the class pass
static int pack_fill_info(hsk_ctx* k, hsk_volume_info* f) {
  memset(f, 0, sizeof(*f));
  f->flags = k->d_color ? 1u : 0u;
  f->dims[0] = k->vp.X;
  f->dims[1] = k->vp.Y;
  f->dims[2] = k->vp.Z;
  f->z0 = k->vp.zs0;
  f->nz = k->vp.nzs;
  for (int i = 0; i < 3; ++i) f->size_m[i] = k->vp.size[i];
  f->trunc_dist_m = k->cfg.trunc_dist_m;
  f->trunc_eff_m = k->vp.tau;
  f->width = k->cfg.width;
  f->height = k->cfg.height;
  f->fx = k->cfg.fx;
  f->fy = k->cfg.fy;
  f->cx = k->cfg.cx;
  f->cy = k->cfg.cy;
  int r = download_state(k);
  if (r != HSK_OK) return r;
  rt_to_pose16(k->h_st->R, k->h_st->t, f->pose);
  f->frame = k->frame;
  f->color_max_weight = k->d_color ? k->color_max_w : 0;
  f->color_band_m = k->d_color ? k->color_band : 0.0f;
  return HSK_OK;
}

extern "C" int hsk_pack_volume(hsk_ctx* k, void* buf, size_t cap_bytes, size_t* n_bytes, hsk_volume_info* info) {
  if (!k) return HSK_ERR_ARG;
  if (!n_bytes) return fail(k, HSK_ERR_ARG, "hsk_pack_volume: n_bytes is null");
  int r = pack_state_check(k, "hsk_pack_volume");
  if (r != HSK_OK) return r;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  flush_weights(k);  // the image holds weights
  r = ensure_pack(k);
  if (r != HSK_OK) return r;
  const PackBufs pb = pack_bufs(k);
  const bool colour = k->d_color != nullptr;
  const bool reused = k->pack.stands_for(k, &colour, sizeof(colour));
  if (!reused) {
    k->pack.drop();
    launch_pack_classify(k->stream, k->d_vol, k->vp, pb.cls_t, pb.off_t);
    launch_pack_scan(k->stream, pb.off_t, pb.n_bricks, pb.bsum, pb.counts);
    if (colour) {
      launch_pack_classify_color(k->stream, k->d_color, k->vp, pb.cls_c, pb.off_c);
      launch_pack_scan(k->stream, pb.off_c, pb.n_bricks, pb.bsum, pb.counts + 8);
    }
    HIPCHK(k, hipGetLastError());
    HIPCHK(k, hipMemcpyAsync(k->pk_counts, pb.counts, 64, hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    k->pack.stamp(k, &colour, sizeof(colour));
  }
  hsk_volume_info f;
  r = pack_fill_info(k, &f);
  if (r != HSK_OK) return r;
  for (int i = 0; i < 4; ++i) f.tsdf_bricks[i] = k->pk_counts[i];
  if (colour) {
    f.color_bricks[0] = k->pk_counts[8];
    f.color_bricks[1] = k->pk_counts[8 + 3];
  }
  hskv_finish_info(&f);
  f.pass_reused = reused ? 1 : 0;
  if (f.tsdf_payload_bytes != (uint64_t)k->pk_counts[4] * 4 || (colour && f.color_payload_bytes != (uint64_t)k->pk_counts[8 + 4] * 4))
    return fail(k, HSK_ERR_STATE, "hsk_pack_volume: the class counts and the scanned payload length disagree");
  *n_bytes = (size_t)f.total_bytes;
  if (info) *info = f;
  if (!buf) return HSK_OK;
  if (cap_bytes < f.total_bytes) return fail(k, HSK_ERR_ARG, "hsk_pack_volume: the buffer is smaller than the image");
  r = ensure_product_bytes(k, (size_t)f.total_bytes);
  if (r != HSK_OK) return r;
  // the image in the product buffer: header, class table, payload (, colour class table, colour payload)
  char* img = (char*)k->d_out;
  unsigned char head[HSKV_HEADER_BYTES];
  hskv_write_header(&f, head);
  r = ensure_pinned(k);
  if (r != HSK_OK) return r;
  memcpy(k->h_pin[0], head, HSKV_HEADER_BYTES);
  HIPCHK(k, hipMemcpyAsync(img, k->h_pin[0], HSKV_HEADER_BYTES, hipMemcpyHostToDevice, k->stream));
  size_t at = HSKV_HEADER_BYTES;
  HIPCHK(k, hipMemcpyAsync(img + at, pb.cls_t, pb.table_bytes, hipMemcpyDeviceToDevice, k->stream));
  at += pb.table_bytes;
  launch_pack_gather(k->stream, k->d_vol, false, k->vp, pb.cls_t, pb.off_t, img + at);
  at += (size_t)f.tsdf_payload_bytes;
  if (colour) {
    HIPCHK(k, hipMemcpyAsync(img + at, pb.cls_c, pb.table_bytes, hipMemcpyDeviceToDevice, k->stream));
    at += pb.table_bytes;
    launch_pack_gather(k->stream, k->d_color, true, k->vp, pb.cls_c, pb.off_c, img + at);
  }
  HIPCHK(k, hipGetLastError());
  return copy_out(k, buf, k->d_out, (size_t)f.total_bytes);
}

extern "C" int hsk_unpack_volume(hsk_ctx* k, const void* buf, size_t n_bytes) {
  if (!k) return HSK_ERR_ARG;
  if (!buf) return fail(k, HSK_ERR_ARG, "hsk_unpack_volume: buf is null");
  int r = pack_state_check(k, "hsk_unpack_volume");
  if (r != HSK_OK) return r;
  hsk_volume_info f;
  std::string why;
  if (hskv_validate(buf, n_bytes, &f, &why) != HSK_OK) return fail(k, HSK_ERR_ARG, why.c_str());
  if (f.dims[0] != k->vp.X || f.dims[1] != k->vp.Y || f.dims[2] != k->vp.Z || f.z0 != k->vp.zs0 || f.nz != k->vp.nzs)
    return fail(k, HSK_ERR_ARG, "hsk_unpack_volume: the image's dims or stored planes are not the context's");
  if (memcmp(f.size_m, k->vp.size, sizeof(f.size_m)) != 0) return fail(k, HSK_ERR_ARG, "hsk_unpack_volume: the image's size_m is not the context's");
  if (memcmp(&f.trunc_eff_m, &k->vp.tau, sizeof(float)) != 0)
    return fail(k, HSK_ERR_ARG, "hsk_unpack_volume: the image's effective truncation distance is not the context's (stored TSDF values are in units of it)");
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  r = ensure_pack(k);
  if (r == HSK_OK) r = ensure_pinned(k);
  if (r != HSK_OK) return r;
  const PackBufs pb = pack_bufs(k);
  const bool colour = (f.flags & 1u) != 0u && k->d_color != nullptr;
  const size_t payload_t = (size_t)f.tsdf_payload_bytes, payload_c = colour ? (size_t)f.color_payload_bytes : 0;
  r = ensure_product_bytes(k, payload_t + payload_c + 512);
  if (r != HSK_OK) return r;
  k->pack.drop();  // the pack tables are about to hold the image's classes
  const unsigned char* src = (const unsigned char*)buf;
  // a host range into device memory, in pieces through the pinned pair; `turn` counts the pieces of this call
  int turn = 0;
  auto upload = [&](void* dst_dev, const unsigned char* from, size_t bytes) -> int {
    return stage_in(k, &turn, from, bytes, k->pin_bytes, [&](void* pin, size_t off, size_t len) -> int {
      HIPCHK(k, hipMemcpyAsync((char*)dst_dev + off, pin, len, hipMemcpyHostToDevice, k->stream));
      return HSK_OK;
    });
  };
  char* pay_t = (char*)k->d_out;
  char* pay_c = pay_t + ((payload_t + 255) & ~(size_t)255);
  size_t at = HSKV_HEADER_BYTES;
  r = upload(pb.cls_t, src + at, pb.table_bytes);
  if (r != HSK_OK) return r;
  at += pb.table_bytes;
  launch_pack_sizes(k->stream, pb.cls_t, pb.n_bricks, pb.off_t);
  launch_pack_scan(k->stream, pb.off_t, pb.n_bricks, pb.bsum, pb.counts);
  r = upload(pay_t, src + at, payload_t);
  if (r != HSK_OK) return r;
  at += payload_t;
  HIPCHK(k, hipMemsetAsync(k->d_vol, 0, k->vol_bytes, k->stream));  // ZERO bricks and the padding planes
  launch_pack_scatter(k->stream, k->d_vol, false, k->vp, pb.cls_t, pb.off_t, pay_t);
  if (k->d_color) HIPCHK(k, hipMemsetAsync(k->d_color, 0, k->color_bytes, k->stream));
  if (colour) {
    r = upload(pb.cls_c, src + at, pb.table_bytes);
    if (r != HSK_OK) return r;
    at += pb.table_bytes;
    launch_pack_sizes(k->stream, pb.cls_c, pb.n_bricks, pb.off_c);
    launch_pack_scan(k->stream, pb.off_c, pb.n_bricks, pb.bsum, pb.counts + 8);
    r = upload(pay_c, src + at, payload_c);
    if (r != HSK_OK) return r;
    launch_pack_scatter(k->stream, k->d_color, true, k->vp, pb.cls_c, pb.off_c, pay_c);
  }
  HIPCHK(k, hipGetLastError());
  r = volume_replaced(k);
  if (r != HSK_OK) return r;
  HIPCHK(k, hipStreamSynchronize(k->stream));
  HIPCHK(k, hipGetLastError());
  return HSK_OK;
}

extern "C" int hsk_save_volume(hsk_ctx* k, const char* path, hsk_volume_info* info) {
  if (!k) return HSK_ERR_ARG;
  if (!path) return fail(k, HSK_ERR_ARG, "hsk_save_volume: path is null");
  size_t n = 0;
  hsk_volume_info f;
  int r = hsk_pack_volume(k, nullptr, 0, &n, &f);
  if (r != HSK_OK) return r;
  std::vector<unsigned char> img;
  try {
    img.resize(n);
  } catch (const std::bad_alloc&) {
    return fail(k, HSK_ERR_STATE, "hsk_save_volume: out of host memory for the image");
  }
  r = hsk_pack_volume(k, img.data(), n, &n, &f);
  if (r != HSK_OK) return r;
  const std::string tmp = std::string(path) + ".tmp";
  FILE* fp = fopen(tmp.c_str(), "wb");
  if (!fp) return fail(k, HSK_ERR_STATE, "hsk_save_volume: cannot create the file");
  const bool ok = fwrite(img.data(), 1, n, fp) == n;
  const bool closed = fclose(fp) == 0;
  if (!ok || !closed || rename(tmp.c_str(), path) != 0) {
    (void)remove(tmp.c_str());
    return fail(k, HSK_ERR_STATE, "hsk_save_volume: cannot write the file");
  }
  if (info) *info = f;
  return HSK_OK;
}

extern "C" int hsk_load_volume(hsk_ctx* k, const char* path) {
  if (!k) return HSK_ERR_ARG;
  if (!path) return fail(k, HSK_ERR_ARG, "hsk_load_volume: path is null");
  const int rs = pack_state_check(k, "hsk_load_volume");
  if (rs != HSK_OK) return rs;
  FILE* fp = fopen(path, "rb");
  if (!fp) return fail(k, HSK_ERR_STATE, "hsk_load_volume: cannot open the file");
  std::vector<unsigned char> img;
  bool ok = fseeko(fp, 0, SEEK_END) == 0;
  const long long len = ok ? (long long)ftello(fp) : -1;
  ok = ok && len >= 0 && fseeko(fp, 0, SEEK_SET) == 0;
  if (ok) {
    try {
      img.resize((size_t)len);
    } catch (const std::bad_alloc&) {
      fclose(fp);
      return fail(k, HSK_ERR_STATE, "hsk_load_volume: out of host memory for the file");
    }
    ok = fread(img.data(), 1, img.size(), fp) == img.size();
  }
  fclose(fp);
  if (!ok) return fail(k, HSK_ERR_STATE, "hsk_load_volume: cannot read the file");
  return hsk_unpack_volume(k, img.data(), img.size());
}

extern "C" int hsk_volume_image_info(const void* buf, size_t n_bytes, hsk_volume_info* info) {
  if (!buf || !info) {
    create_error() = "hsk_volume_image_info: null argument";
    return HSK_ERR_ARG;
  }
  return hskv_validate(buf, n_bytes, info, &create_error());
}
extern "C" int hsk_volume_file_info(const char* path, hsk_volume_info* info) {
  if (!path || !info) {
    create_error() = "hsk_volume_file_info: null argument";
    return HSK_ERR_ARG;
  }
  return hskv_validate_file(path, info, &create_error());
}
extern "C" int hsk_config_from_volume(const hsk_volume_info* info, hsk_config* c) {
  if (!info || !c) {
    create_error() = "hsk_config_from_volume: null argument";
    return HSK_ERR_ARG;
  }
  hsk_default_config(c, info->dims[0]);
  c->vol_x = info->dims[0];
  c->vol_y = info->dims[1];
  c->vol_z = info->dims[2];
  for (int i = 0; i < 3; ++i) c->vol_size_m[i] = info->size_m[i];
  c->trunc_dist_m = info->trunc_dist_m;
  c->width = info->width;
  c->height = info->height;
  c->fx = info->fx;
  c->fy = info->fy;
  c->cx = info->cx;
  c->cy = info->cy;
  memcpy(c->init_pose, info->pose, sizeof(c->init_pose));
  c->own_z0 = 0;
  c->own_z1 = info->dims[2];
  return HSK_OK;
}

extern "C" int hsk_resume_scan(hsk_ctx* k, const float pose[16]) {
  if (!k) return HSK_ERR_ARG;
  if (!pose) return fail(k, HSK_ERR_ARG, "hsk_resume_scan: pose is null");
  int r = pack_state_check(k, "hsk_resume_scan");  // (a slab's model maps are composited from every slab's march)
  if (r != HSK_OK) return r;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  leave_slab_bookkeeping(k);
  r = download_state(k);
  if (r != HSK_OK) return r;
  // the state a tracked frame at `pose` leaves: its pose (the next frame's ICP starts from it and takes it as the previous
  // one), not lost, nothing to reset
  pose16_to_rt(pose, k->h_st->R, k->h_st->t);
  pose16_to_rt(pose, k->h_st->Rp, k->h_st->tp);
  k->h_st->lost = 0;
  k->h_st->need_reset = 0;
  r = upload_state(k);
  if (r != HSK_OK) return r;
  enqueue_raycast_and_resize(k, nullptr);  // the model maps of all three levels, as the frame's own raycast makes them
  HIPCHK(k, hipStreamSynchronize(k->stream));
  HIPCHK(k, hipGetLastError());
  k->pending_reset = false;
  if (k->frame < 1) k->frame = 1;
  return HSK_OK;
}

