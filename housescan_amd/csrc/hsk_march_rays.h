// hsk_march_rays.h -- FUNCTION-BODY TEXT, included inside a march kernel behind hsk_march_stage.h (see hsk_march.h), second
// piece: the pinhole ray of pixel (x, y) and where it enters and leaves the volume's box; hsk_march_loop.h follows.
//   in : what hsk_march_stage.h left, in_img (the lane's pixel lies in the image), vp, in (Intr), and st: a pointer to
//        anything with the camera's pose as float R[9], t[3] (cam->world) -- the TrackState, or a view's camera block
//   out: vx, vy, vz, nx, ny, nz, key (all still "none"), i (the pixel's index, 0 outside the image), P = W * H, the ray o + d * time
//        as t0, t1, t2, d0, d1, d2, and t_start, t_exit
  const size_t P = (size_t)W * H;
  const size_t i = in_img ? (size_t)y * W + x : 0;
  float vx = HSK_NANF, vy = HSK_NANF, vz = HSK_NANF, nx = HSK_NANF, ny = HSK_NANF, nz = HSK_NANF;
  int key = HSK_KEY_NONE_I;

  const float t0 = st->t[0], t1 = st->t[1], t2 = st->t[2];
  const float rx = ((float)x - in.cx) / in.fx, ry = ((float)y - in.cy) / in.fy;
  float d0 = (st->R[0] * rx + st->R[1] * ry) + st->R[2] * 1.0f;
  float d1 = (st->R[3] * rx + st->R[4] * ry) + st->R[5] * 1.0f;
  float d2 = (st->R[6] * rx + st->R[7] * ry) + st->R[8] * 1.0f;
  const float inv = 1.0f / sqrtf(hsk_dot3(d0, d1, d2, d0, d1, d2));
  d0 = d0 * inv;
  d1 = d1 * inv;
  d2 = d2 * inv;
  if (d0 == 0.0f) d0 = 1e-15f;
  if (d1 == 0.0f) d1 = 1e-15f;
  if (d2 == 0.0f) d2 = 1e-15f;
  const float tmin0 = ((d0 > 0.0f ? 0.0f : vp.size[0]) - t0) / d0, tmax0 = ((d0 > 0.0f ? vp.size[0] : 0.0f) - t0) / d0;
  const float tmin1 = ((d1 > 0.0f ? 0.0f : vp.size[1]) - t1) / d1, tmax1 = ((d1 > 0.0f ? vp.size[1] : 0.0f) - t1) / d1;
  const float tmin2 = ((d2 > 0.0f ? 0.0f : vp.size[2]) - t2) / d2, tmax2 = ((d2 > 0.0f ? vp.size[2] : 0.0f) - t2) / d2;
  float t_start = fmaxf(fmaxf(tmin0, tmin1), tmin2);
  const float t_exit = fminf(fminf(tmax0, tmax1), tmax2);
  t_start = fmaxf(t_start, 0.0f);
