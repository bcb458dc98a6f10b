// reloc.hip -- pose scoring for gfx950 (hsk_score_cloud, hsk_relocalize; DESIGN.md 3.13 the kernel, 8g the rule): how well
// does a cloud, moved by each of many candidate poses, lie on the surfaces a volume's TSDF holds.
//
// The rule (tests/reloc_twin.py restates it in numpy): a point (x, y, z) is moved by the pose,
// p_i = ((R[i][0] x + R[i][1] y) + R[i][2] z) + t[i], sampled once with the raycast's trilinear sample (hsk_sample.h) and
// falls in exactly one of six classes (hsk_reloc_point.h); a near point adds rint(|F| 2^16) to the pose's sum_abs.  Every
// sum is an integer, so any order of addition gives the same bits, and nothing here is atomic:
//
// k_reloc_score: a grid of poses x point slabs.  The pose is the block's -- blockIdx.x -- so its 12 floats arrive by scalar
// loads and stay in SGPRs; the block strides over the cloud's three planes (coalesced) from its slab on; a lane is a point:
// eight 4-B gathers.  The class counts are the wave's: one ballot and one population count per class and 64 points, in
// scalar registers (the skipped ones are what remains of the points the wave took).  sum_abs is a lane's integer, one
// butterfly adds it at the end.  The block's four waves meet in 256 B of LDS and eight lanes store the block's eight values
// to [pose][slab] with plain vector stores.
// k_reloc_sum: a lane per pose adds its slabs (at most HSK_RELOC_MAX_SLABS) and writes the pose's hsk_pose_score.
//
// k_reloc_gather: the cloud of a frame for hsk_relocalize -- every `stride`-th pixel of a vertex map and its normal, the
// normal turned to face the camera (n . v > 0: negated), as the alignment's six planes.
#pragma clang fp contract(off)
#include "../../include/hskinfu.h"
#include "hsk_dev.h"
#include "hsk_cloud_dev.h"
#include "hsk_launch.h"
#include "hsk_reloc_point.h"

__global__ __launch_bounds__(256) void k_reloc_score(const unsigned* __restrict__ vol, const float* __restrict__ soa,
                                                     const float* __restrict__ poses, SampleVol dv, unsigned n, unsigned pitch,
                                                     unsigned long long* __restrict__ partial) {
  const unsigned pose = blockIdx.x, slab = blockIdx.y, n_slabs = gridDim.y;
  const float* __restrict__ P = poses + (size_t)pose * 12u;  // uniform over the block: scalar loads
  float R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = P[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = P[9 + i];
  unsigned cnt[RELOC_SKIPPED] = {0u, 0u, 0u, 0u, 0u}, taken = 0u;  // the wave's (uniform)
  long long sum = 0;                                                 // the lane's
  const unsigned wave_off = threadIdx.x & ~63u;
  for (unsigned base = slab * 256u; base < n; base += n_slabs * 256u) {
    const unsigned i = base + threadIdx.x;
    const bool act = i < n;
    const CloudPos p = hsk_cloud_pos(soa, hsk_cloud_at(act, i, n), pitch);
    unsigned q;
    int cls = reloc_point(vol, dv, R, t, p.x, p.y, p.z, q);
    cls = act ? cls : -1;
    sum += act ? (long long)q : 0ll;
#pragma unroll
    for (int c = 0; c < RELOC_SKIPPED; ++c) cnt[c] += (unsigned)__popcll(__ballot(cls == c));
    const unsigned wb = base + wave_off;
    taken += wb < n ? (n - wb < 64u ? n - wb : 64u) : 0u;
  }
  sum = hsk_wave_sum(sum);
  unsigned long long mine[8];  // the wave's eight words
  unsigned rest = taken;
#pragma unroll
  for (int c = 0; c < RELOC_SKIPPED; ++c) {
    mine[c] = cnt[c];
    rest -= cnt[c];
  }
  mine[RELOC_SKIPPED] = rest;
  mine[6] = (unsigned long long)sum;
  mine[7] = 0ull;
  const unsigned long long r = hsk_block_meet<HskSum>(mine);
  if (threadIdx.x < 8u) partial[((size_t)pose * n_slabs + slab) * 8u + threadIdx.x] = r;
}

__global__ __launch_bounds__(256) void k_reloc_sum(const unsigned long long* __restrict__ partial, unsigned n_poses, unsigned n_slabs,
                                                   hsk_pose_score* __restrict__ out) {
  const unsigned pose = blockIdx.x * 256u + threadIdx.x;
  if (pose >= n_poses) return;
  unsigned long long v[8] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
  for (unsigned s = 0; s < n_slabs; ++s) {
    const unsigned long long* __restrict__ p = partial + ((size_t)pose * n_slabs + s) * 8u;
#pragma unroll
    for (int c = 0; c < 7; ++c) v[c] += p[c];
  }
  hsk_pose_score sc;
  sc.n_near = (unsigned)v[RELOC_NEAR];
  sc.n_free = (unsigned)v[RELOC_FREE];
  sc.n_behind = (unsigned)v[RELOC_BEHIND];
  sc.n_unseen = (unsigned)v[RELOC_UNSEEN];
  sc.n_outside = (unsigned)v[RELOC_OUTSIDE];
  sc.n_skipped = (unsigned)v[RELOC_SKIPPED];
  sc.sum_abs = v[6];
  out[pose] = sc;
}

unsigned reloc_slabs(unsigned n, unsigned n_poses) {
  // slabs only where the poses alone do not fill the device: 8192 blocks in all, then a block takes the whole cloud
  const unsigned by_points = (n + 255u) / 256u, by_poses = n_poses >= 8192u ? 1u : 8192u / (n_poses ? n_poses : 1u);
  unsigned s = by_points < by_poses ? by_points : by_poses;
  s = s < (unsigned)HSK_RELOC_MAX_SLABS ? s : (unsigned)HSK_RELOC_MAX_SLABS;
  return s ? s : 1u;
}

void launch_reloc_score(hipStream_t s, const void* dst_vol, const VolParams& dv, const float* soa, unsigned n, unsigned pitch,
                        const float* poses12, unsigned n_poses, unsigned long long* partial, hsk_pose_score* scores) {
  if (n == 0 || n_poses == 0) return;
  const unsigned n_slabs = reloc_slabs(n, n_poses);
  hipLaunchKernelGGL(k_reloc_score, dim3(n_poses, n_slabs), dim3(256), 0, s, (const unsigned*)dst_vol, soa, poses12, hsk_sample_vol(dv),
                     n, pitch, partial);
  hipLaunchKernelGGL(k_reloc_sum, dim3((n_poses + 255u) / 256u), dim3(256), 0, s, partial, n_poses, n_slabs, scores);
}

__global__ __launch_bounds__(256) void k_reloc_gather(const float* __restrict__ vmap, const float* __restrict__ nmap, unsigned P,
                                                      unsigned stride, unsigned np, unsigned pitch, float* __restrict__ soa) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= np) return;
  const size_t at = (size_t)i * stride;  // (< P: np = ceil(P / stride))
  const float x = vmap[at], y = vmap[P + at], z = vmap[2 * (size_t)P + at];
  float nx = nmap[at], ny = nmap[P + at], nz = nmap[2 * (size_t)P + at];
  const bool turn = hsk_dot3(nx, ny, nz, x, y, z) > 0.0f;  // facing away from the camera at the origin
  nx = turn ? -nx : nx;
  ny = turn ? -ny : ny;
  nz = turn ? -nz : nz;
  soa[i] = x;
  soa[pitch + i] = y;
  soa[2 * (size_t)pitch + i] = z;
  soa[3 * (size_t)pitch + i] = nx;
  soa[4 * (size_t)pitch + i] = ny;
  soa[5 * (size_t)pitch + i] = nz;
}

void launch_reloc_gather(hipStream_t s, const float* vmap, const float* nmap, unsigned P, unsigned stride, unsigned np, unsigned pitch,
                         float* soa) {
  if (np == 0) return;
  hipLaunchKernelGGL(k_reloc_gather, dim3((np + 255u) / 256u), dim3(256), 0, s, vmap, nmap, P, stride, np, pitch, soa);
}
