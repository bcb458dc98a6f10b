// hsk_march_loop.h -- FUNCTION-BODY TEXT, included inside a march kernel behind a ray piece (hsk_march_rays.h, or a kernel's own:
// section.hip), third piece: the march through the volume and the deferred refinement of the hits.  Nothing of
// the camera is used here but the ray.
//   in : what hsk_march_stage.h left; from the ray piece vx .. nz, key (NaN / none), i, P, the ray t0, t1, t2 (origin: uniform or
//        per lane), d0, d1, d2 (unit, no component 0), t_start, t_exit and in_img (false: the lane's ray does not march); vol, vp, SLAB
//   out: vx, vy, vz, nx, ny, nz (NaN: no hit / no normal), key
  {
    const float ic0 = 1.0f / vp.cell[0], ic1 = 1.0f / vp.cell[1], ic2 = 1.0f / vp.cell[2];
    const int bs = vp.bshift;
    const int bxn = vp.X >> bs, byn = vp.Y >> bs;
    const float time_step = vp.tau * 0.8f;
    const float max_time = 3.0f * ((vp.size[0] + vp.size[1]) + vp.size[2]);
    float time_curr = t_start;
    int step = 0;
    // near sample of step 0: the entry voxel, clamped into the grid (A.6)
    int qx = vox_fast(t0 + d0 * time_curr, vp.cell[0], ic0);
    int qy = vox_fast(t1 + d1 * time_curr, vp.cell[1], ic1);
    int qz = vox_fast(t2 + d2 * time_curr, vp.cell[2], ic2);
    int px = qx < 0 ? 0 : (qx > vp.X - 1 ? vp.X - 1 : qx);
    int py = qy < 0 ? 0 : (qy > vp.Y - 1 ? vp.Y - 1 : qy);
    int pz = qz < 0 ? 0 : (qz > vp.Z - 1 ? vp.Z - 1 : qz);
    bool crossing = false;
    int nux = 0, nuy = 0, nuz = 0;  // unclamped voxel of the near sample at the crossing
    // brick flag of a voxel inside the grid (0 when its plane is not stored by this slab)
    auto flag_at = [&](int vx_, int vy_, int vz_) -> unsigned {
      const int zz = SLAB ? vz_ - vp.zs0 : vz_;
      const bool stored = !SLAB || (zz >= 0 && zz < vp.nzs);
      const int bf = __mul24(__mul24(stored ? (zz >> bs) : 0, byn) + (vy_ >> bs), bxn) + (vx_ >> bs);
      const unsigned w = lflags[bf >> 5];
      return stored ? ((w >> (bf & 31)) & 1u) : 0u;
    };
    {
      uint4* dst = (uint4*)lflags;
      if (q0 < nq) dst[q0] = a0;
      if (q1 < nq) dst[q1] = a1;
      if (q2 < nq) dst[q2] = a2;
      if (q3 < nq) dst[q3] = a3;
      for (int q = threadIdx.x + RC_STAGE_MAX * RC_BLOCK; q < nq; q += RC_BLOCK) ((uint4*)lflags)[q] = ((const uint4*)flags)[q];
    }
    __syncthreads();
    RC_STAMP(1);
    unsigned fl_prev = flag_at(px, py, pz);  // always the flag of the current near sample
    // Voxel of a sample: the spec's floor(p / cell).  q = p * (1 / cell) differs from the correctly rounded quotient
    // by < 3 * 2^-24 * |q|, so both have the same floor unless q lies within eps of an integer -- for every q inside
    // or within a voxel of the grid; a sample farther out is outside the grid either way (its error is relative).
    const float eps = 3.0e-7f * (float)max(vp.X, max(vp.Y, vp.Z)) + 1.0e-5f;
    bool first = true;  // the near sample of the first step is the (clamped) entry voxel; qx,qy,qz hold it unclamped
    // voxel of the far sample at ray parameter tn (floor(p / cell) of the spec); false when it lies outside the grid
    auto far_voxel = [&](float tn, int& gx, int& gy, int& gz) -> bool {
      const float pnx = t0 + d0 * tn, pny = t1 + d1 * tn, pnz = t2 + d2 * tn;
      const float q0 = pnx * ic0, q1 = pny * ic1, q2 = pnz * ic2;
      const float r0 = __builtin_amdgcn_fractf(q0), r1 = __builtin_amdgcn_fractf(q1), r2 = __builtin_amdgcn_fractf(q2);
      float f0 = q0 - r0, f1 = q1 - r1, f2 = q2 - r2;  // floor
      // distance of the fractional parts from 1/2: far from 1/2 means close to an integer
      const float far_from_half = fmaxf(fmaxf(fabsf(r0 - 0.5f), fabsf(r1 - 0.5f)), fabsf(r2 - 0.5f));
      if (!(far_from_half < 0.5f - eps)) {  // rare (or NaN): the exact floor(p / cell) of the spec
        f0 = floorf(pnx / vp.cell[0]);
        f1 = floorf(pny / vp.cell[1]);
        f2 = floorf(pnz / vp.cell[2]);
      }
      // v_cvt_i32_f32 saturates; a negative or huge index fails the unsigned bound test
      gx = (int)f0;
      gy = (int)f1;
      gz = (int)f2;
      return ((unsigned)gx < (unsigned)vp.X) & ((unsigned)gy < (unsigned)vp.Y) & ((unsigned)gz < (unsigned)vp.Z);  // (no short circuit: no lane-mask branch)
    };
#ifdef HSK_RC_TIMING
    unsigned trips = 0, gtrips = 0;        // acted steps; acted steps that compared voxels (per lane)
    unsigned it_all = 0, it_skip = 0, it_empty = 0;  // loop iterations; crossings; regular trips in which no lane gathered (wave)
#endif
    // The march advances RC_GROUP steps per trip.  A step that lies next to a flagged brick needs its two voxels, and a
    // wave whose lanes reach such bricks at different steps used to stop for a memory round trip (~0.9 us under load) at
    // every step in which ANY lane gathered (tools/rc_timing.sh: march time = 0.06 us x steps + 0.9 us x gather steps +
    // 46 us of waiting for other lanes' gathers).  Here the far samples of the next RC_GROUP steps are located first
    // (voxel + brick flag: arithmetic and LDS only), then every voxel any of those steps will compare is loaded in
    // one batch -- the same voxels the step-by-step march reads, no others -- and the steps are then acted on in order
    // with the values in registers: one round trip per RC_GROUP steps instead of up to RC_GROUP.  Same decisions, same
    // ray parameters ((time_curr + time_step) + time_step ...), so the maps are bit-identical.
    bool ended = !(in_img && t_start < t_exit);
    // Crossing clear super-bricks: when the near sample of EVERY marching lane of the wave sits in a super-brick (4^3
    // bricks) none of whose bricks has held a negative TSDF, and every lane's ray stays inside its super-brick for the
    // next RC_SKIP steps and RC_MARGIN of a step more, none of those steps can gather or end -- their only effect is to
    // advance time_curr and step.  So the wave advances them by the same float additions and looks up the new near
    // sample once.  The decision is wave-wide (the 64 rays of an 8x8 tile are a few centimetres apart, so they cross the
    // same super-bricks together; per-lane skipping made every trip pay for both paths: raycast_analysis.md).
    const bool can_skip = !SLAB && hsk_super_ok(vp);
    const int ss = bs + HSK_SUPER_SHIFT, sxn = hsk_super_dim(vp.X, bs), syn = hsk_super_dim(vp.Y, bs), szn = hsk_super_dim(vp.Z, bs);
    const float s_edge0 = (float)(1 << ss) * vp.cell[0], s_edge1 = (float)(1 << ss) * vp.cell[1], s_edge2 = (float)(1 << ss) * vp.cell[2];
    const float id0 = 1.0f / d0, id1 = 1.0f / d1, id2 = 1.0f / d2;
    const float inv_step = 1.0f / time_step;
    // (a wave-wide loop: lanes whose ray has ended idle inside it, so that the wave-wide minimum below can use shuffles)
    RC_STAMP(6);
    while (__ballot(!ended && time_curr < max_time) != 0ull) {
      const bool act = !ended && time_curr < max_time;
#ifdef HSK_RC_TIMING
      ++it_all;
#endif
      if (can_skip) {
        // Steps every marching lane can cross at once at one level of the block hierarchy (sh: log2 of the block edge in
        // voxels; xn, yn, zn: blocks per axis; woff: where the level's bits start in lflags; half: its edge is half a
        // super-brick's): 0 unless the near sample of EVERY marching lane sits in a clear block.
        auto crossing_steps = [&](const int sh, const int xn, const int yn, const int zn, const int woff, const bool half) -> int {
          const int s0 = px >> sh, s1 = py >> sh, s2 = pz >> sh;
          const int sbit = (s2 * yn + s1) * xn + s0;
          const bool clear = !((lflags[woff + (sbit >> 5)] >> (sbit & 31)) & 1u);
          // (one ballot settles the common "no": the waves that graze a surface for a hundred steps -- the ones the launch
          // ends with -- must not pay for exit distances and a wave-wide minimum at every trip)
          if (__ballot(act && !clear) != 0ull) return 0;
          const float g0 = half ? 0.5f * s_edge0 : s_edge0, g1 = half ? 0.5f * s_edge1 : s_edge1, g2 = half ? 0.5f * s_edge2 : s_edge2;
          // ray parameter at which the ray leaves the block (approximate; RC_MARGIN of a step absorbs the error)
          float e0 = ((float)(s0 + (d0 > 0.0f ? 1 : 0)) * g0 - t0) * id0;
          float e1 = ((float)(s1 + (d1 > 0.0f ? 1 : 0)) * g1 - t1) * id1;
          float e2 = ((float)(s2 + (d2 > 0.0f ? 1 : 0)) * g2 - t2) * id2;
          float te = fminf(fminf(e0, e1), e2);
#if RC_EXT > 0
          // ... and on through up to RC_EXT further blocks while they are clear too (open air: the regular trip that used
          // to carry the march across every face between two clear blocks is most of what a room costs).  The next block
          // is the one behind the face the ray leaves by; that is certain only when the runner-up face lies clearly later
          // (near an edge or corner the float exit times may order wrongly, and the ray could cut through a third, flagged
          // block): RC_TIE = 1/16 step = 1.5 mm, a thousand times what the exit times can be off by (a few ulp of a few
          // metres); otherwise the crossing ends here.  (Two steps, the first choice, ended a fifth of the crossings early:
          // 58.9 -> 57.4 us.)
          {
            int c0 = s0, c1 = s1, c2 = s2;
            bool live = act;
#pragma unroll
            for (int k = 0; k < RC_EXT; ++k) {
              const bool a0 = e0 <= e1 && e0 <= e2, a1 = !a0 && e1 <= e2, a2 = !a0 && !a1;
              const float second = a0 ? fminf(e1, e2) : (a1 ? fminf(e0, e2) : fminf(e0, e1));
              const int n0 = c0 + (a0 ? (d0 > 0.0f ? 1 : -1) : 0), n1 = c1 + (a1 ? (d1 > 0.0f ? 1 : -1) : 0),
                        n2 = c2 + (a2 ? (d2 > 0.0f ? 1 : -1) : 0);
              live = live && (second - te >= RC_TIE * time_step) && (unsigned)n0 < (unsigned)xn && (unsigned)n1 < (unsigned)yn &&
                     (unsigned)n2 < (unsigned)zn;
              const int nb = live ? (n2 * yn + n1) * xn + n0 : 0;
              live = live && !((lflags[woff + (nb >> 5)] >> (nb & 31)) & 1u);
              if (live) {
                c0 = n0; c1 = n1; c2 = n2;
                e0 = a0 ? e0 + g0 * fabsf(id0) : e0;
                e1 = a1 ? e1 + g1 * fabsf(id1) : e1;
                e2 = a2 ? e2 + g2 * fabsf(id2) : e2;
                te = fminf(fminf(e0, e1), e2);
              }
            }
          }
#endif
          const float room = (te - time_curr) * inv_step - RC_MARGIN;
          return wave_min_i32(!act ? 0x7fffffff : (room >= 1.0f ? (int)fminf(room, RC_SKIP_MAX) : 0));
        };
        int n = crossing_steps(ss, sxn, syn, szn, flag_words, false);
        if (n >= RC_SKIP && n != 0x7fffffff) {  // wave-uniform
          float tc = time_curr;
          int i_ = 0;
          for (; i_ + 4 <= n; i_ += 4) tc = (((tc + time_step) + time_step) + time_step) + time_step;  // (the march's own additions, in order)
          for (; i_ < n; ++i_) tc = tc + time_step;
          int nx_, ny_, nz_;
          const bool fine = !act || (far_voxel(tc, nx_, ny_, nz_) && tc < max_time);
          if (__ballot(!fine) == 0ull) {
            if (act) {
              time_curr = tc;
              step += n;
              px = nx_; py = ny_; pz = nz_;
              first = false;
              fl_prev = flag_at(px, py, pz);
            }
#ifdef HSK_RC_TIMING
            ++it_skip;
#endif
            continue;
          }
        }
      }
      if (!act) continue;
      float tt[RC_GROUP];
      int vx_[RC_GROUP], vy_[RC_GROUP], vz_[RC_GROUP];
      bool okv[RC_GROUP], need[RC_GROUP];
      unsigned fl[RC_GROUP];
      bool all_alive;
      {
        float tc = time_curr;
        bool alive = true;
        unsigned fprev = fl_prev;
#pragma unroll
        for (int g = 0; g < RC_GROUP; ++g) {
          alive = alive && (tc < max_time);
          tt[g] = tc + time_step;
          okv[g] = far_voxel(tt[g], vx_[g], vy_[g], vz_[g]);
          alive = alive && okv[g];
          fl[g] = flag_at(alive ? vx_[g] : 0, alive ? vy_[g] : 0, alive ? vz_[g] : 0);  // (looked up whether alive or not: no branch)
          fl[g] = alive ? fl[g] : 0u;
          const bool owned = !SLAB || (vz_[g] >= vp.zo0 && vz_[g] < vp.zo1);
          need[g] = alive && owned && ((fprev | fl[g]) != 0u);
          fprev = fl[g];
          tc = tt[g];
        }
        all_alive = alive;
      }
      bool any_need = false;
#pragma unroll
      for (int g = 0; g < RC_GROUP; ++g) any_need = any_need || need[g];
      // Most trips outside the clear super-bricks still compare nothing (a flagged super-brick is mostly unflagged
      // bricks): when every marching lane's RC_GROUP steps stay inside the grid, before max_time and away from flagged
      // bricks, acting on them one by one comes to this.
      if (__ballot(!(all_alive && !any_need)) == 0ull) {
        px = vx_[RC_GROUP - 1]; py = vy_[RC_GROUP - 1]; pz = vz_[RC_GROUP - 1];
        first = false;
        fl_prev = fl[RC_GROUP - 1];
        time_curr = tt[RC_GROUP - 1];
        step += RC_GROUP;
#ifdef HSK_RC_TIMING
        trips += RC_GROUP;
        ++it_empty;
#endif
        continue;
      }
      int raw[RC_GROUP + 1];  // raw[0]: the near sample of the first step; raw[g + 1]: the far sample of step g
#pragma unroll
      for (int g = 0; g <= RC_GROUP; ++g) raw[g] = 0;
      if (any_need) {
        if (need[0]) raw[0] = raw_at(vol, vp, px, py, pz);
#pragma unroll
        for (int g = 0; g < RC_GROUP; ++g)
          if (need[g] || (g + 1 < RC_GROUP && need[g + 1])) raw[g + 1] = raw_at(vol, vp, vx_[g], vy_[g], vz_[g]);
      }
      // Acting on the RC_GROUP steps in order, without branches: a step halts the lane when the march is past max_time, the
      // far sample lies outside the grid (the ray ends), or the two voxels show a back face or a zero crossing; the steps
      // before the first halt advance the lane.  (With a divergent branch and a break per step this was 85 instructions a
      // step, most of them lane-mask bookkeeping; the same decisions as selects are 15.)
      {
        bool run = true, e_out = false, e_back = false, e_cross = false;
        int adv = 0;
#pragma unroll
        for (int g = 0; g < RC_GROUP; ++g) {
          const float tcur = g == 0 ? time_curr : tt[g - 1];
          const bool on = run && (tcur < max_time);
          const bool back = need[g] && raw[g] < 0 && raw[g + 1] > 0;
          const bool cross = need[g] && raw[g] > 0 && raw[g + 1] < 0;
          e_out = e_out || (on && !okv[g]);
          e_back = e_back || (on && okv[g] && back);
          e_cross = e_cross || (on && okv[g] && cross);
          run = on && okv[g] && !back && !cross;
          // the far sample of an advancing step is the next step's near sample
          px = run ? vx_[g] : px;
          py = run ? vy_[g] : py;
          pz = run ? vz_[g] : pz;
          fl_prev = run ? fl[g] : fl_prev;
          time_curr = run ? tt[g] : time_curr;
          adv += run ? 1 : 0;
#ifdef HSK_RC_TIMING
          trips += on ? 1 : 0;
          gtrips += (on && okv[g] && need[g]) ? 1 : 0;
#endif
        }
        const bool was_first = first && adv == 0;
        first = first && adv == 0;
        step += adv;
        if (e_back) key = (step << 1) | 1;
        if (e_cross) {  // zero crossing: refined below with every lane of the wave; (px, py, pz) is the near sample of its step
          crossing = true;
          nux = was_first ? qx : px;
          nuy = was_first ? qy : py;
          nuz = was_first ? qz : pz;
        }
        ended = ended || e_out || e_back || e_cross;
      }
    }
    // Deferred hit processing: lanes hit at different steps, and refining inside the loop would run these
    // (memory-latency-bound) taps once per distinct step.  Here the wave runs them once, loads batched.
    RC_STAMP(2);
#ifdef HSK_RC_TIMING
    {
      // wave totals: the longest lane's trips, and the number of lanes-trips with gathers (max over lanes)
      unsigned tmax = trips, gmax = gtrips, ia = it_all, is = it_skip, ie = it_empty;
      for (int o = 32; o > 0; o >>= 1) {
        tmax = max(tmax, (unsigned)__shfl_xor((int)tmax, o, 64));
        gmax = max(gmax, (unsigned)__shfl_xor((int)gmax, o, 64));
        ia = max(ia, (unsigned)__shfl_xor((int)ia, o, 64));
        is = max(is, (unsigned)__shfl_xor((int)is, o, 64));
        ie = max(ie, (unsigned)__shfl_xor((int)ie, o, 64));
      }
      if (lane == (int)__builtin_ctzll(__ballot(true)) && tile_id < 8192) {
        g_rc_times[tile_id * 8 + 4] = tmax;
        g_rc_times[tile_id * 8 + 5] = (unsigned long long)(gmax & 0xffffu) | ((unsigned long long)(ia & 0xffffu) << 16) |
                                      ((unsigned long long)(is & 0xffffu) << 32) | ((unsigned long long)(ie & 0xffffu) << 48);
      }
    }
#endif
    if (crossing) {
      key = (step << 1) | 1;
      const float tn = time_curr + time_step;
      const float Ftdt = trilinear(vol, vp, t0 + d0 * tn, t1 + d1 * tn, t2 + d2 * tn);
      const float Ft = trilinear(vol, vp, t0 + d0 * time_curr, t1 + d1 * time_curr, t2 + d2 * time_curr);
      if (!hsk_isnan(Ftdt) && !hsk_isnan(Ft)) {
        const float Ts = time_curr - (time_step * Ft) / (Ftdt - Ft);
        if (Ts >= time_curr - time_step && Ts <= time_curr + 2.0f * time_step) {  // (D3: two steps round the far sample)
          vx = t0 + d0 * Ts;
          vy = t1 + d1 * Ts;
          vz = t2 + d2 * Ts;
          key = (step << 1);
          if (nux > 1 && nuy > 1 && nuz > 1 && nux < vp.X - 2 && nuy < vp.Y - 2 && nuz < vp.Z - 2) {
            const float xp = trilinear(vol, vp, vx + vp.cell[0], vy, vz), xm = trilinear(vol, vp, vx - vp.cell[0], vy, vz);
            const float yp = trilinear(vol, vp, vx, vy + vp.cell[1], vz), ym = trilinear(vol, vp, vx, vy - vp.cell[1], vz);
            const float zp = trilinear(vol, vp, vx, vy, vz + vp.cell[2]), zm = trilinear(vol, vp, vx, vy, vz - vp.cell[2]);
            const float gxn = xp - xm, gyn = yp - ym, gzn = zp - zm;
            const float ninv = 1.0f / sqrtf(hsk_dot3(gxn, gyn, gzn, gxn, gyn, gzn));
            nx = gxn * ninv;
            ny = gyn * ninv;
            nz = gzn * ninv;
          }
        }
      }
    }
  }
