// hsk_march.h -- what the TSDF march's kernels share (raycast.hip: k_raycast, the tracker's model frame; view.hip:
// k_render_view, a scene image from any camera; section.hip: k_render_section): the voxel look-up, the trilinear sample (also
// the normals of extract.hip), the march's constants and its wave-wide minimum.  The march itself is three pieces of
// function-body text -- hsk_march_stage.h, hsk_march_rays.h (the pinhole ray) and hsk_march_loop.h -- that each kernel includes at
// its place; section.hip puts its own ray piece between the stage and the loop.  The sample's arithmetic -- where the point
// lies among the voxel centres, the eight-term sum -- is hsk_sample.h's, shared with fusion and alignment; what is the
// march's own here is the slab handling round it.  k_raycast's machine code is the bar for any change to either file: it must
// not move (tools/isa_compare.py against a build of the parent).
#pragma once
#include "hsk_dev.h"
// ------------------------------------------------------------------------------------------------------
// raycast (A.6).  One ray per lane; a wave covers an 8x8 pixel tile so that neighbouring rays walk
// neighbouring voxels (L1/L2 locality of the 4-B gathers).  Steps are owned by the slab that contains the
// far sample's z plane; a single-device context owns all of them.
// ------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ int raw_at(const short2* __restrict__ vol, const VolParams& vp, int x, int y, int z) {
  const int zz = z - vp.zs0;
  if (zz < 0 || zz >= vp.nzs) return 0;
  // (block row and pitch are below 2^24 each: one 24-bit multiply-add forms the row, one widening multiply-add the index --
  // hsk_vox_index in the fewest instructions: these sit on the march's gather chain)
  const unsigned row = __umul24((unsigned)zz >> 2, (unsigned)vp.Y) + (unsigned)y;
  const unsigned low = ((((unsigned)x & ~3u) | ((unsigned)zz & 3u)) << 2) | ((unsigned)x & 3u);
  return (int)vol[(size_t)row * (unsigned)((vp.X >> 2) << 4) + low].x;
}

// trilinear TSDF sample (A.6).  Branch-free: indices are clamped for the loads and the NaN of the spec
// (sample on the outer shell of the grid) is selected at the end, so that the 8 taps of several calls can be
// in flight together.
static __device__ __forceinline__ float trilinear(const short2* __restrict__ vol, const VolParams& vp, float px, float py,
                                                  float pz) {
  const SampleCell sc = hsk_sample_cell(vp, px, py, pz);
  const int gx = sc.x, gy = sc.y, gz = sc.z;
  // stored planes: a tap outside the slab reads plane 0 of the slab and is discarded (cannot happen when the
  // halo is sized as DESIGN.md prescribes)
  const int z0 = gz - vp.zs0, z1 = z0 + 1;
  const bool in0 = z0 >= 0 && z0 < vp.nzs, in1 = z1 >= 0 && z1 < vp.nzs;
  // (the index is a sum of one term per axis: two terms per axis, eight additions; the two z taps of a cell share a
  // 64-B block three times out of four)
  // the upper neighbours' terms by steps from the lower ones: +1 word in x (or to the next block: +13), one row pitch in y,
  // +4 words in z (or to the next block row of planes: + the plane-group pitch - 12); a z tap outside the stored planes
  // reads plane 0 (term 0: z0 = -1 gives z1 = 0) and is discarded
  const size_t pitch = (size_t)((vp.X >> 2) << 4);
  const size_t tx0 = hsk_vox_xterm(gx), tx1 = tx0 + ((gx & 3) == 3 ? 13u : 1u);
  const size_t ty0 = (size_t)gy * pitch, ty1 = ty0 + pitch;
  const size_t tz0 = in0 ? hsk_vox_zterm(vp, z0) : 0;
  const size_t tz1 = (in0 && in1) ? tz0 + ((z0 & 3) == 3 ? (size_t)vp.Y * pitch - 12u : 4u) : 0;
  const int r000 = vol[tz0 + ty0 + tx0].x, r100 = vol[tz0 + ty0 + tx1].x, r010 = vol[tz0 + ty1 + tx0].x, r110 = vol[tz0 + ty1 + tx1].x;
  const int r001 = vol[tz1 + ty0 + tx0].x, r101 = vol[tz1 + ty0 + tx1].x, r011 = vol[tz1 + ty1 + tx0].x, r111 = vol[tz1 + ty1 + tx1].x;
  const float f000 = hsk_tsdf_unpack(in0 ? r000 : 0), f100 = hsk_tsdf_unpack(in0 ? r100 : 0);
  const float f010 = hsk_tsdf_unpack(in0 ? r010 : 0), f110 = hsk_tsdf_unpack(in0 ? r110 : 0);
  const float f001 = hsk_tsdf_unpack(in1 ? r001 : 0), f101 = hsk_tsdf_unpack(in1 ? r101 : 0);
  const float f011 = hsk_tsdf_unpack(in1 ? r011 : 0), f111 = hsk_tsdf_unpack(in1 ? r111 : 0);
  const float f[8] = {f000, f100, f010, f110, f001, f101, f011, f111};
  const float res = hsk_sample_blend(f, sc.a, sc.b, sc.c);  // (unconditionally: a select, not a branch)
  return sc.in ? res : HSK_NANF;
}

// floor(p / cell) of the spec without the IEEE division in the common case: q = p * (1/cell) differs from the
// correctly rounded quotient by < 3 * 2^-24 * |q|, so unless q sits within 2.5e-4 of an integer (|q| < 1100)
// both have the same floor; the rare lanes that do sit there take the exact division.
static __device__ __forceinline__ int vox_fast(float p, float cell, float inv_cell) {
  const float q = p * inv_cell;
  float f = floorf(q);
  const float fr = q - f;
  if (!(fr > 2.5e-4f && fr < 0.99975f && q > -1100.0f && q < 1100.0f)) f = floorf(p / cell);
  if (!(f >= 0.0f)) return -1;
  if (f > 1.0e6f) return 1000000;
  return (int)f;
}

#ifndef RC_BLOCK
#define RC_BLOCK 64     // one wave = one 8x8 tile = one workgroup with its own 4 KiB copy of the brick bitfield: the 4800
#endif                  // waves of a 640x480 frame spread evenly over the SIMDs.  Measured 512^3 / 1024^3 (us): 64 threads
                        // 99 / 124, 128: 107 / 126, 256: 99 / 131, 512: 107 / 142.  With 512-thread blocks and a 32 KiB
                        // bitfield 88 of the 256 CUs got a third block and the kernel waited for them (raycast_analysis.md).
#ifndef RC_WPE
#define RC_WPE 5  // waves per SIMD the register allocator must leave room for (96 VGPRs): the 4800 tiles of a 640x480 frame are all resident at five (5120 slots), and six would cost spills
#endif
#ifndef RC_EXT
#define RC_EXT 2       // further clear super-bricks a crossing may run on through
#endif
#define RC_SKIP_MAX (64.0f * (RC_EXT + 1))  // most steps crossed at once
#ifndef RC_MARGIN
#define RC_MARGIN 0.125f  // steps a crossing stops short of the last face (3 mm: the exit times and the accumulated ray parameter are
#endif                    // good to micrometres; two whole steps, the first choice, cost every crossing two steps: 57.3 -> 56.5 us)
#ifndef RC_TIE
#define RC_TIE 0.0625f  // steps by which the runner-up face must lie behind the first for a crossing to run on through it
#endif
#ifndef RC_SKIP
#define RC_SKIP 2      // fewest steps worth crossing at once inside a clear super-brick
#endif
#ifndef RC_GROUP
#define RC_GROUP 4     // march steps located and gathered together (k_raycast)
#endif
// A wave's pixel tile is TW x (64 / TW), a template parameter of the kernel (round 5; profiles/r05/raycast_notes.md): 8 x 8,
// or 16 x 4 for volumes far beyond the Infinity Cache -- x-adjacent rays gather x-adjacent voxels, four of which share a
// 64-B block: 1024^3 71.6 -> 66.3 us, 512^3 56.8 -> 57.1 (kept at 8 x 8); 4 x 16: 60.8 / 84.6 us.
#define RC_TH (64 / RC_TW)
#define RC_STAGE_MAX 4  // 16-B loads per thread: 4 KiB / (64 x 16 B); larger bitfields take the loop below
// minimum over the 64 lanes of a wave whose lanes are ALL active, as a wave-uniform value: four DPP steps inside each row of
// 16 lanes, two row broadcasts, one v_readlane (six ds_bpermute round trips through the LDS crossbar before)
static __device__ __forceinline__ int wave_min_i32(int v) {
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false));  // row_half_mirror
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false));  // row_mirror: every lane holds its row's minimum
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false));  // row_bcast:15 into rows 1 and 3
  v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false));  // row_bcast:31 into rows 2 and 3
  return __builtin_amdgcn_readlane(v, 63);
}
