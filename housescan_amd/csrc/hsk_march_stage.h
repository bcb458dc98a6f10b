// hsk_march_stage.h -- FUNCTION-BODY TEXT, included inside a march kernel (see hsk_march.h), first piece: the brick bitfield's
// loads are requested and the wave's pixel is found.
//   in : flags, flag_words, W, H (locals of the kernel), RC_TW (the tile width), RC_STAMP (a macro; empty unless the kernel is timed)
//   out: lflags (the LDS array), nq, q0..q3, a0..a3 (the bitfield on its way), lane, tile, tiles_x, tiles_y, x, y
  // the whole brick bitfield ("this brick has held a negative TSDF") lives in LDS: the march then touches
  // global memory only next to surfaces
  extern __shared__ unsigned lflags[];
#ifdef HSK_RC_TIMING
  const int tile_id = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  RC_STAMP(0);
#endif
  // The bitfield is REQUESTED here -- 16-B loads, all of a thread's loads in flight at once (a one-word-at-a-time staging
  // loop cost 9 us per block: profiles/r01/raycast_analysis.md) -- and put into LDS further down, behind the ray set-up,
  // which needs none of it: at the start of a launch every wave of the chip is at this point at once, and nothing else
  // is there to run under the loads.
  const int nq = (flag_words + HSK_SUPER_WORDS) >> 2;  // brick bits + super-brick bits, both multiples of 4 words
  // (an indexed temporary array here was placed in scratch memory by the compiler: named registers instead)
  const int q0 = threadIdx.x, q1 = q0 + RC_BLOCK, q2 = q1 + RC_BLOCK, q3 = q2 + RC_BLOCK;
  static_assert(RC_STAGE_MAX == 4, "the staging is written for four 16-B loads per thread");
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  const uint4 a0 = q0 < nq ? ((const uint4*)flags)[q0] : zero4;
  const uint4 a1 = q1 < nq ? ((const uint4*)flags)[q1] : zero4;
  const uint4 a2 = q2 < nq ? ((const uint4*)flags)[q2] : zero4;
  const uint4 a3 = q3 < nq ? ((const uint4*)flags)[q3] : zero4;
#ifndef HSK_RC_TIMING
  const int lane = threadIdx.x & 63;
#endif
  const int tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int tiles_x = (W + RC_TW - 1) / RC_TW, tiles_y = (H + RC_TH - 1) / RC_TH;
  // Tile rows are dispatched from the top and bottom edges of the image inwards (0, last, 1, last - 1, ...): the rays of
  // the border rows meet floor and ceiling at grazing angles and march longest, and a wave dispatched last onto a SIMD
  // that already holds its share of waves finishes last -- with the rows in image order the launch ended with exactly
  // those tiles (tools/rc_timing.sh).  Scheduling only.  Measured 512^3 / 1024^3: 90.6 / 117.9 -> 86.8 / 110.8 us.
  const int ty_lin = tile / tiles_x;
  const int ty = (ty_lin & 1) ? (tiles_y - 1 - (ty_lin >> 1)) : (ty_lin >> 1);
  const int x = (tile % tiles_x) * RC_TW + (lane % RC_TW);
  const int y = ty * RC_TH + (lane / RC_TW);
