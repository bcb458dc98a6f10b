// hsk_cover_point.h -- scan coverage, the work on ONE probe ray under ONE pose (DESIGN.md 8i the rule, 3.15 the kernels): a
// voxel's observation state from its pair word, the voxel a sample of the ray falls in, the ray's state machine as a step
// function, and the whole ray as cover.hip's kernels walk it.  Like hsk_reloc_point.h it is plain C++ with no HIP type in it,
// so that tests/cover_point_harness.cpp compiles the same text for the host and tests/test_cover_host.py compares it with the
// numpy twin (tests/cover_twin.py) ray for ray, without a GPU.  One rounding per written operator: both builds forbid contraction.
#pragma once
#include "hsk_sample.h"

// a voxel's state, in the order of hsk_view_score's eye_state (3: the point lies outside the grid)
#define COVER_FREE 0    // observed (weight != 0) and raw > 0
#define COVER_UNSEEN 1  // weight == 0
#define COVER_SOLID 2   // observed and raw <= 0
#define COVER_NOWHERE 3

// a ray's class, in the order of hsk_view_score's counts
#define COVER_HIT 0
#define COVER_FRONTIER 1
#define COVER_OPEN 2
#define COVER_BLIND 3
#define COVER_OUTSIDE 4
#define COVER_CLASSES 5

// the ray's state between two samples; from COVER_RS_HIT on the ray has ended
#define COVER_RS_START 0     // no sample was inside so far
#define COVER_RS_FREE 1      // every inside sample so far was FREE
#define COVER_RS_FRONTIER 2  // decided by an UNSEEN sample and going on: its gain is still counted
#define COVER_RS_HIT 3
#define COVER_RS_BLIND 4
#define COVER_RS_OPEN 5          // left the grid behind FREE samples
#define COVER_RS_FRONTIER_END 6  // a FRONTIER ray's count stopped (a SOLID or an outside sample)

#define COVER_MAX_SAMPLES 4096

HSK_HD int cover_state(unsigned word) { return hsk_pair_wgt(word) == 0 ? COVER_UNSEEN : hsk_pair_raw(word) > 0 ? COVER_FREE : COVER_SOLID; }

// (state, the sample's voxel state, the sample lies inside the grid) -> state; an ended ray stays as it is
HSK_HD int cover_next(int rs, int s, bool inside) {
  const int from_start = !inside ? COVER_RS_START : s == COVER_FREE ? COVER_RS_FREE : COVER_RS_BLIND;
  const int from_free = !inside ? COVER_RS_OPEN : s == COVER_FREE ? COVER_RS_FREE : s == COVER_SOLID ? COVER_RS_HIT : COVER_RS_FRONTIER;
  const int from_frontier = (!inside || s == COVER_SOLID) ? COVER_RS_FRONTIER_END : COVER_RS_FRONTIER;
  return rs == COVER_RS_START ? from_start : rs == COVER_RS_FREE ? from_free : rs == COVER_RS_FRONTIER ? from_frontier : rs;
}
HSK_HD bool cover_running(int rs) { return rs < COVER_RS_HIT; }
// the class a ray ends in, from the state its last sample left
HSK_HD int cover_class(int rs) {
  return rs == COVER_RS_START ? COVER_OUTSIDE
         : (rs == COVER_RS_FREE || rs == COVER_RS_OPEN) ? COVER_OPEN
         : rs == COVER_RS_HIT ? COVER_HIT
         : rs == COVER_RS_BLIND ? COVER_BLIND
                                : COVER_FRONTIER;
}

// a ray on its way: the state, the UNSEEN samples counted so far and the sample that decided it (-1: none yet)
struct CoverRay {
  int rs;
  unsigned gain;
  int decided;
};
HSK_HD CoverRay cover_ray_begin(bool live) {
  CoverRay r;
  r.rs = live ? COVER_RS_START : COVER_RS_OPEN;  // (a lane without a ray: ended, and counted nowhere by its caller)
  r.gain = 0u;
  r.decided = -1;
  return r;
}
// sample i of the ray: the step, and what hangs on it -- a FREE ray's first non-FREE sample decides it; a FRONTIER ray counts
// its UNSEEN samples from that one on
HSK_HD void cover_ray_step(CoverRay& r, int i, int s, bool inside) {
  const int next = cover_next(r.rs, s, inside);
  r.decided = (r.rs == COVER_RS_FREE && (next == COVER_RS_HIT || next == COVER_RS_FRONTIER)) ? i : r.decided;
  r.gain += (next == COVER_RS_FRONTIER && s == COVER_UNSEEN) ? 1u : 0u;  // (only an inside sample keeps a ray in FRONTIER)
  r.rs = next;
}

// the probe as a kernel takes it: the fields of hsk_probe and the number of samples, computed once on the host
struct CoverProbe {
  int W, H, n;
  float fx, fy, cx, cy, near_m, step_m;
};
// n = min(4096, floor((far - near) / step) + 1) in binary64 from the binary32 fields (far >= near >= 0, step > 0: n >= 1)
static inline int cover_sample_count(float near_m, float far_m, float step_m) {
  const double q = floor(((double)far_m - (double)near_m) / (double)step_m) + 1.0;
  return q >= (double)COVER_MAX_SAMPLES ? COVER_MAX_SAMPLES : (int)q;
}

// a pixel's ray direction at depth 1, and the depth of sample i along the optical axis
HSK_HD float cover_dir(int pix, float c, float f) { return ((float)pix - c) / f; }
HSK_HD float cover_depth(const CoverProbe& pr, int i) { return pr.near_m + (float)i * pr.step_m; }
// rint(z * 1000) millimetres when that lies within 1..65535, else 0
HSK_HD unsigned cover_depth_mm(float z) {
  const float mm = rintf(z * 1000.0f);
  return (mm >= 1.0f && mm <= 65535.0f) ? (unsigned)mm : 0u;
}

// Where sample (dx z, dy z, z) of the pose (R, t) lies: the voxel's word index in the block layout (hsk_dev.h: hsk_vox_index;
// a volume holds fewer than 2^32 words), of the voxel clamped into the grid so that the load is legal whatever the point is -- a
// NaN, an infinity, kilometres away -- and `inside`: the unclamped voxel lies in the grid (a NaN does not).
template <class Vol>
HSK_HD unsigned cover_voxel_word(const Vol& v, float px, float py, float pz, bool& inside) {
  const int gx = hsk_vox_of_q(hsk_div_by_const(px, v.icell[0])), gy = hsk_vox_of_q(hsk_div_by_const(py, v.icell[1])),
            gz = hsk_vox_of_q(hsk_div_by_const(pz, v.icell[2]));
  inside = gx >= 0 && gx < v.X && gy >= 0 && gy < v.Y && gz >= 0 && gz < v.Z;
  const unsigned x = (unsigned)hsk_min_i(hsk_max_i(gx, 0), v.X - 1), y = (unsigned)hsk_min_i(hsk_max_i(gy, 0), v.Y - 1),
                 z = (unsigned)hsk_min_i(hsk_max_i(gz, 0), v.Z - 1);
  const unsigned pitch = (unsigned)((v.X >> 2) << 4);
  return ((z >> 2) * (unsigned)v.Y * pitch + ((z & 3u) << 2)) + y * pitch + (((x >> 2) << 4) + (x & 3u));
}
template <class Vol>
HSK_HD unsigned cover_sample_word(const Vol& v, const float* R, const float* t, float dx, float dy, float z, bool& inside) {
  const float x = dx * z, y = dy * z;
  const float p0 = ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
  const float p1 = ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
  const float p2 = ((R[6] * x + R[7] * y) + R[8] * z) + t[2];
  return cover_voxel_word(v, p0, p1, p2, inside);
}

// the state of the voxel that holds the camera centre t (COVER_NOWHERE: outside the grid)
template <class Vol>
HSK_HD int cover_eye_state(const unsigned* vol, const Vol& v, const float* t) {
  bool inside;
  const unsigned at = cover_voxel_word(v, t[0], t[1], t[2], inside);
  const int s = cover_state(vol[at]);
  return inside ? s : COVER_NOWHERE;
}

// The samples of one ray are gathered COVER_GROUP at a time: a sample's address depends on the pose and the pixel alone, only the
// state machine depends on the sample before it, so the loads of a group are issued together and then acted on in order (the
// march's RC_GROUP, hsk_march_loop.h) -- one memory round trip per group instead of one per sample.
#define COVER_GROUP 8
#if defined(__HIPCC__)
#define COVER_UNROLL _Pragma("unroll")
#else
#define COVER_UNROLL
#endif
// samples [i0, i0 + COVER_GROUP) of one ray, those below pr.n
template <class Vol>
HSK_HD void cover_ray_group(const unsigned* vol, const Vol& v, const CoverProbe& pr, const float* R, const float* t, float dx, float dy,
                            int i0, CoverRay& r) {
  unsigned w[COVER_GROUP];
  bool in[COVER_GROUP];
COVER_UNROLL
  for (int g = 0; g < COVER_GROUP; ++g) {
    const int i = hsk_min_i(i0 + g, pr.n - 1);  // (past the end: the last sample again, and not acted on)
    w[g] = vol[cover_sample_word(v, R, t, dx, dy, cover_depth(pr, i), in[g])];
  }
COVER_UNROLL
  for (int g = 0; g < COVER_GROUP; ++g)
    if (i0 + g < pr.n) cover_ray_step(r, i0 + g, cover_state(w[g]), in[g]);
}

// one whole ray, as the host harness walks it (the kernels run the same groups, a wave at a time): its class, gain and depth
template <class Vol>
HSK_HD int cover_ray(const unsigned* vol, const Vol& v, const CoverProbe& pr, const float* R, const float* t, int pu, int pv, unsigned& gain,
                     unsigned& depth_mm) {
  const float dx = cover_dir(pu, pr.cx, pr.fx), dy = cover_dir(pv, pr.cy, pr.fy);
  CoverRay r = cover_ray_begin(true);
  for (int i0 = 0; i0 < pr.n && cover_running(r.rs); i0 += COVER_GROUP) cover_ray_group(vol, v, pr, R, t, dx, dy, i0, r);
  gain = r.gain;
  depth_mm = r.decided >= 0 ? cover_depth_mm(cover_depth(pr, r.decided)) : 0u;
  return cover_class(r.rs);
}
