// align.hip -- volume alignment for gfx950 (hsk_align_cloud; DESIGN.md 3.12 the kernel, 8f the rule): one iteration's sums of the
// registration of a cloud with normals against a volume's TSDF.
//
// The rule (tests/align_twin.py restates it in numpy): a source point (x, y, z) with normal n is moved by the
// current matrix, p_i = ((R[i][0] x + R[i][1] y) + R[i][2] z) + t[i], n likewise without t.  The probes j = 0, +1, -1, .., +J, -J
// look at a = p + ((float)j tau) n with the raycast's trilinear sample F (hsk_sample.h: the same guards, cell choice,
// fractions and summation order), the smallest weight Ws of its eight taps and the gradient g of the trilinear form from the
// same eight values, divided by the cells.  A probe is valid when the sample is not the shell's NaN, Ws > 0, |F| < 1, g.g > 0
// and n . g / |g| >= cos_gate; the valid probe with the smallest |F| (the earliest on a tie) gives the point's row
// [q x nd, nd, r], q = p - centre, nd = g / |g|, r = s_j c_j - F tau.  The 27 sums of the ICP's packed upper triangle and the
// sum of r r are taken over rint(row[a] row[b] 2^26) in binary64, integers all, so any order of addition gives the same bits.
//
// Cost: a lane per point, persistent waves striding over the cloud; the six planes of the cloud are read coalesced.  A probe
// is eight 4-B gathers (both halves of the pair: the TSDF and the weight) from the block layout (hsk_dev.h: hsk_vox_index);
// the cloud arrives in voxel order, so neighbouring lanes probe neighbouring voxels.  The probes of a wave share one
// instruction stream: the indices are clamped for the loads, validity is one predicate and the running best is updated by
// selects (hsk_align_point.h: the work on one point, shared with a host harness of the tests).  A lane keeps its 28 sums
// in binary64 registers (integers below 2^53) over all its points; at the wave's end they
// become 64-bit integers, one butterfly adds them over the wave and 29 lanes add one value each into a shard of the
// accumulators.
#pragma clang fp contract(off)
#include "hsk_dev.h"
#include "hsk_cloud_dev.h"
#include "hsk_launch.h"
#include "hsk_align_point.h"

__global__ __launch_bounds__(256) void k_align_iter(const unsigned* __restrict__ vol, const float* __restrict__ soa, SampleVol dv,
                                                    AlignArgs aa, unsigned long long* __restrict__ acc_out) {
  const int lane = threadIdx.x & 63;
  const unsigned n_threads = gridDim.x * 256u;
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0.0;
  unsigned n_used = 0;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < aa.n; i += n_threads) {
    const CloudPoint q = hsk_cloud_point(soa, i, aa.pitch);
    if (align_point(vol, dv, aa, q.x, q.y, q.z, q.nx, q.ny, q.nz, acc)) n_used += 1;
  }
  // a lane's sums are integers below 2^53; over the wave and over the launch they are added as 64-bit integers
  long long mine = 0;
#pragma unroll
  for (int k = 0; k < 29; ++k) {
    const long long t = hsk_wave_sum(k < 28 ? (long long)acc[k] : (long long)n_used);
    mine = lane == k ? t : mine;
  }
  const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (lane < 29 && mine != 0) atomicAdd(&acc_out[(wave % HSK_ALIGN_SHARDS) * 32u + (unsigned)lane], (unsigned long long)mine);
}

void launch_align_iter(hipStream_t s, const void* dst_vol, const VolParams& dv, const float* soa, unsigned n, unsigned pitch,
                       const AlignPose& m, int probes, float cos_gate, unsigned long long* acc) {
  if (n == 0) return;
  const SampleVol av = hsk_sample_vol(dv);
  AlignArgs aa;
  for (int i = 0; i < 3; ++i) {
    aa.t[i] = m.t[i];
    aa.c[i] = dv.size[i] * 0.5f;
  }
  for (int i = 0; i < 9; ++i) aa.R[i] = m.R[i];
  aa.tau = dv.tau;
  aa.cos_gate = cos_gate;
  aa.J = probes;
  aa.n = n;
  aa.pitch = pitch;
  // persistent waves: a lane per point up to a few waves per SIMD of the device, then the lanes stride
  const unsigned want = (n + 255u) / 256u;
  const unsigned blocks = want < 2048u ? want : 2048u;
  hipLaunchKernelGGL(k_align_iter, dim3(blocks), dim3(256), 0, s, (const unsigned*)dst_vol, soa, av, aa, acc);
}
