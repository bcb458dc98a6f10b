// normals.hip -- cloud normals for gfx950 (hsk_estimate_normals; DESIGN.md 3.28 the kernels, 8v the rule): a fixed-radius neighbour
// search over a cloud in the alignment scratch's planes (hsk_cloud_dev.h), built on the device, and hsk_normal_point.h's solve.
//   k_normal_keys:    a lane a point -- its cell's key claimed in an open-addressing table by a 64-bit compare-and-swap, the
//                     cell's count raised once per wave and cell (the wave's lanes of one cell folded first)
//   (launch_scan_rows: the cells' counts into their first slots)
//   k_normal_scatter: a lane a point -- its q and its index into its cell's range; the order inside a cell is arrival order and
//                     nothing reads it but integer sums.  The invalid points get their outputs here.
//   k_normal_gather:  a lane a point IN CELL ORDER, so that a wave's lanes walk the same few ranges -- the 27 cells around its own
//                     looked up, the ten sums, the solve, the outputs at the point's original index
// Every loop is bounded by its inputs: a probe by the table's size, a walk by the cells' counts; no block waits for another.  A
// probe that runs out raises the error word (words[NORMAL_W_ERROR]) and the call fails; nothing spins.
#pragma clang fp contract(off)
#include "hsk_cloud_dev.h"
#include "hsk_launch.h"
#include "hsk_normal_point.h"

#define NORMAL_NO_SLOT 0xFFFFFFFFu

// The wave's active lanes that hold the same slot, as one group: `rank` this lane's place in its group (by lane number), `size` the
// group's lanes, `first` its lowest lane.  Every lane of the wave arrives; at most 64 trips, one per group.
static __device__ __forceinline__ void normal_wave_groups(bool act, unsigned slot, unsigned& rank, unsigned& size, unsigned& first) {
  const unsigned lane = threadIdx.x & 63u;
  unsigned long long todo = __ballot(act);
  rank = size = 0u;
  first = lane;
  for (int trip = 0; trip < 64 && todo != 0ull; ++trip) {
    const unsigned head = (unsigned)__ffsll((long long)todo) - 1u;
    const unsigned s = __shfl(slot, (int)head, 64);
    const unsigned long long same = __ballot(act && slot == s) & todo;
    if ((same >> lane) & 1ull) {
      rank = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
      size = (unsigned)__popcll(same);
      first = head;
    }
    todo &= ~same;
  }
}

// the slot of `key` in the table, or NORMAL_NO_SLOT: the key is not there (*lost stays) or the probe ran out (*lost = true)
static __device__ __forceinline__ unsigned normal_find(const unsigned long long* __restrict__ keys, unsigned mask, unsigned long long key, bool* lost) {
  unsigned s = normal_hash(key, mask);
  for (unsigned probe = 0u; probe <= mask; ++probe) {
    const unsigned long long k = keys[s];
    if (k == key) return s;
    if (k == NORMAL_KEY_EMPTY) return NORMAL_NO_SLOT;
    s = (s + 1u) & mask;
  }
  *lost = true;
  return NORMAL_NO_SLOT;
}

static __device__ __forceinline__ unsigned long long normal_point_key(const CloudPos& p, int r_q) {
  return normal_key(normal_cell(plane_q(p.x), r_q), normal_cell(plane_q(p.y), r_q), normal_cell(plane_q(p.z), r_q));
}

__global__ __launch_bounds__(256) void k_normal_keys(const float* __restrict__ soa, unsigned n, unsigned pitch, int r_q, NormalIndex ix) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const bool in = i < n;
  const CloudPos p = hsk_cloud_pos(soa, hsk_cloud_at(in, i, n), pitch);
  const bool valid = in && normal_point_valid(p.x, p.y, p.z);
  unsigned slot = NORMAL_NO_SLOT;
  bool fresh = false, lost = false;
  if (valid) {
    const unsigned long long key = normal_point_key(p, r_q);
    unsigned s = normal_hash(key, ix.mask);
    lost = true;
    for (unsigned probe = 0u; probe <= ix.mask; ++probe) {  // (at most the table's size)
      unsigned long long old = __hip_atomic_load(ix.keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old == NORMAL_KEY_EMPTY) {
        old = atomicCAS(ix.keys + s, NORMAL_KEY_EMPTY, key);  // (the slot's key before: ours to claim, or whoever came first)
        fresh = old == NORMAL_KEY_EMPTY;
        if (fresh) old = key;
      }
      if (old == key) {
        slot = s;
        lost = false;
        break;
      }
      s = (s + 1u) & ix.mask;
    }
  }
  if (in) ix.slot[i] = slot;
  unsigned rank, size, first;
  normal_wave_groups(slot != NORMAL_NO_SLOT, slot, rank, size, first);
  if (slot != NORMAL_NO_SLOT && rank == 0u) atomicAdd(ix.counts + slot, size);
  const unsigned cells = (unsigned)__popcll(__ballot(fresh));
  if ((threadIdx.x & 63u) == 0u && cells != 0u) atomicAdd(ix.words + NORMAL_W_CELLS, (unsigned long long)cells);
  if (lost) ix.words[NORMAL_W_ERROR] = 1ull;
}

__global__ __launch_bounds__(256) void k_normal_scatter(const float* __restrict__ soa, unsigned n, unsigned pitch, NormalIndex ix, NormalOut out) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  const bool in = i < n;
  const unsigned slot = in ? ix.slot[i] : NORMAL_NO_SLOT;
  const bool act = slot != NORMAL_NO_SLOT;
  unsigned rank, size, first;
  normal_wave_groups(act, slot, rank, size, first);
  unsigned base = 0u;
  if (act && rank == 0u) base = atomicAdd(ix.cursor + slot, size);
  base = __shfl(base, (int)first, 64);
  if (act) {
    const unsigned long long at = ix.off[slot] + (unsigned long long)(base + rank);
    if (at < (unsigned long long)n) {  // (the cells' counts add up to the valid points: always)
      const CloudPos p = hsk_cloud_pos(soa, i, pitch);
      ix.sq[at] = plane_q(p.x);
      ix.sq[(size_t)pitch + at] = plane_q(p.y);
      ix.sq[2u * (size_t)pitch + at] = plane_q(p.z);
      ix.sidx[at] = i;
    } else {
      ix.words[NORMAL_W_ERROR] = 1ull;
    }
  } else if (in) {
    out.normals[3u * (size_t)i] = out.normals[3u * (size_t)i + 1u] = out.normals[3u * (size_t)i + 2u] = 0.0f;
    out.curvature[i] = 0.0f;
    out.neighbours[i] = 0u;
    out.cls[i] = (unsigned char)NORMAL_INVALID;
  }
  const unsigned invalid = (unsigned)__popcll(__ballot(in && !act));
  if ((threadIdx.x & 63u) == 0u && invalid != 0u) atomicAdd(ix.words + NORMAL_INVALID, (unsigned long long)invalid);
}

__global__ __launch_bounds__(256) void k_normal_gather(const float* __restrict__ soa, unsigned n, unsigned pitch, int r_q, NormalArgs args,
                                                       const float* __restrict__ viewpoints, NormalIndex ix, NormalOut out) {
  const unsigned at = blockIdx.x * 256u + threadIdx.x;
  const unsigned long long total = ix.words[NORMAL_W_VALID];  // (the scan's total, the valid points: at most n)
  const unsigned long long n_valid = total < (unsigned long long)n ? total : (unsigned long long)n;
  long long tally[NORMAL_CLASSES + 1] = {0, 0, 0, 0, 0, 0};  // the classes, then the pairs
  bool lost = false;
  if (at < n && (unsigned long long)at < n_valid) {
    const int qx = ix.sq[at], qy = ix.sq[(size_t)pitch + at], qz = ix.sq[2u * (size_t)pitch + at];
    const unsigned i = ix.sidx[at];
    const int cx = (int)normal_cell(qx, r_q), cy = (int)normal_cell(qy, r_q), cz = (int)normal_cell(qz, r_q);
    const int c_max = (int)normal_cell_max(r_q);
    const normal_i64 r2 = (normal_i64)r_q * (normal_i64)r_q;
    normal_i64 s[NORMAL_SUMS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool full = false;
    // |dq| <= r_q per axis: every neighbour lies in one of the 27 cells around the point's own
    for (int c = 0; c < 27 && !full; ++c) {
      const int nx = cx + c % 3 - 1, ny = cy + (c / 3) % 3 - 1, nz = cz + c / 9 - 1;
      if (nx < 0 || ny < 0 || nz < 0 || nx > c_max || ny > c_max || nz > c_max) continue;
      const unsigned slot = normal_find(ix.keys, ix.mask, normal_key((unsigned)nx, (unsigned)ny, (unsigned)nz), &lost);
      if (slot == NORMAL_NO_SLOT) continue;
      const unsigned long long lo = ix.off[slot];
      unsigned long long hi = lo + (unsigned long long)ix.counts[slot];
      hi = hi < n_valid ? hi : n_valid;
      for (unsigned long long j = lo; j < hi; ++j) {  // (a cell's points: the accepted ones stop at max_neighbours + 1)
        if (normal_add(s, ix.sq[j] - qx, ix.sq[(size_t)pitch + j] - qy, ix.sq[2u * (size_t)pitch + j] - qz, r2) &&
            s[0] > (normal_i64)args.max_neighbours) {
          full = true;
          break;
        }
      }
    }
    float nrm[3] = {0.0f, 0.0f, 0.0f}, curv = 0.0f;
    int cls = normal_count_class(s[0], args.min_neighbours, args.max_neighbours);
    if (cls == NORMAL_OK && i < n) {
      const CloudPos p = hsk_cloud_pos(soa, i, pitch);
      cls = normal_solve(s, p.x, p.y, p.z, viewpoints, (size_t)args.n_viewpoints, args.line_rel, nrm, &curv);
    }
    if (i < n) {
      out.normals[3u * (size_t)i] = nrm[0];
      out.normals[3u * (size_t)i + 1u] = nrm[1];
      out.normals[3u * (size_t)i + 2u] = nrm[2];
      out.curvature[i] = curv;
      out.neighbours[i] = (unsigned)s[0];  // (a CROWDED lane stopped at max_neighbours + 1)
      out.cls[i] = (unsigned char)cls;
    } else {
      lost = true;
    }
#pragma unroll
    for (int k = 0; k < NORMAL_CLASSES; ++k) tally[k] = cls == k ? 1 : 0;
    tally[NORMAL_CLASSES] = s[0];
  }
  if (lost) ix.words[NORMAL_W_ERROR] = 1ull;
#pragma unroll
  for (int k = 0; k <= NORMAL_CLASSES; ++k) tally[k] = hsk_wave_fold<HskSum>(tally[k], k);
  const long long r = hsk_block_meet<HskSum>(tally);
  if (threadIdx.x <= (unsigned)NORMAL_CLASSES && r != 0) atomicAdd(ix.words + threadIdx.x, (unsigned long long)r);
}

void launch_normal_index(hipStream_t s, const float* soa, unsigned n, unsigned pitch, int r_q, const NormalIndex& ix, const NormalOut& out) {
  if (n == 0u) return;
  const unsigned blocks = (n + 255u) / 256u;  // (n <= 2^24: at most 65536 blocks, one trip each)
  k_normal_keys<<<blocks, 256, 0, s>>>(soa, n, pitch, r_q, ix);
  launch_scan_rows(s, ix.counts, ix.off, (int)(ix.mask + 1u), ix.words + NORMAL_W_VALID);
  k_normal_scatter<<<blocks, 256, 0, s>>>(soa, n, pitch, ix, out);
}
void launch_normal_gather(hipStream_t s, const float* soa, unsigned n, unsigned pitch, int r_q, const NormalArgs& args, const float* viewpoints,
                          const NormalIndex& ix, const NormalOut& out) {
  if (n == 0u) return;
  k_normal_gather<<<(n + 255u) / 256u, 256, 0, s>>>(soa, n, pitch, r_q, args, viewpoints, ix, out);
}

// loads this file's code object (hsk_prepare_readout); a hipError_t
int normals_warm() {
  hipFuncAttributes a;
  hipError_t e = hipFuncGetAttributes(&a, (const void*)k_normal_keys);
  if (e == hipSuccess) e = hipFuncGetAttributes(&a, (const void*)k_normal_scatter);
  if (e == hipSuccess) e = hipFuncGetAttributes(&a, (const void*)k_normal_gather);
  return (int)e;
}
