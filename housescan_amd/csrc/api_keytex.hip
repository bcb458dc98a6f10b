// api_keytex.hip -- the C ABI's keyframe textures (include/hskinfu.h "Keyframe textures"; DESIGN.md 3.26 the kernel, 8t the rule):
// the keyframe store (hsk_enable_keyframes, hsk_add_keyframe, hsk_keyframe_count, hsk_get_keyframe, hsk_clear_keyframes,
// hsk_release_keyframes), the host's selection rule (hsk_keyframe_wanted), hsk_default_keytex_params and
// hsk_bake_texture_keyframes, which checks its own parameters and hands the rest to api_texture.hip's texture_bake.  The store is
// one device allocation that nothing but hsk_add_keyframe writes and nothing but the bake's kernel reads: a keyframe goes up as one
// copy of its slot (record, packed colour, depth) on the context's stream.
#pragma clang fp contract(off)
#include <cmath>

#include "hsk_ctx.h"
#include "hsk_keytex_point.h"

static int keytex_state(hsk_ctx* k, const char* who, bool need_store) {
  if (int rs = require_whole_volume(k, k, who, "a keyframe store belongs to a context that stores its whole volume")) return rs;
  if (need_store && !k->d_key) return fail(k, HSK_ERR_STATE, (std::string(who) + ": there is no keyframe store (hsk_enable_keyframes)").c_str());
  return HSK_OK;
}

extern "C" int hsk_enable_keyframes(hsk_ctx* k, int cap, int w, int h) {
  if (!k) return HSK_ERR_ARG;
  if (cap < 1 || cap > KEY_MAX_CAP || w < 2 || w > KEY_MAX_SIDE || h < 2 || h > KEY_MAX_SIDE)
    return fail(k, HSK_ERR_ARG, "hsk_enable_keyframes: cap must lie in 1 .. 255, w and h in 2 .. 4096");
  if (int rs = keytex_state(k, "hsk_enable_keyframes", false)) return rs;
  if (k->d_key) {
    if (cap == k->key_cap && w == k->key_w && h == k->key_h) return HSK_OK;
    return fail(k, HSK_ERR_STATE, "hsk_enable_keyframes: a store of another size exists (hsk_release_keyframes first)");
  }
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  void* d = nullptr;
  HIPCHK(k, hipMalloc(&d, (size_t)cap * key_slot_bytes(w, h)));
  k->d_key = d;
  k->key_cap = cap, k->key_w = w, k->key_h = h, k->key_n = 0;
  k->key_rec.clear();
  return HSK_OK;
}

extern "C" int hsk_add_keyframe(hsk_ctx* k, const uint16_t* depth_mm, const uint8_t* rgb, int w, int h, const float pose[16], const float intr[4],
                                int* index) {
  if (!k) return HSK_ERR_ARG;
  auto refuse = [&](const char* why) { return fail(k, HSK_ERR_ARG, (std::string("hsk_add_keyframe: ") + why).c_str()); };
  if (int rs = keytex_state(k, "hsk_add_keyframe", true)) return rs;
  if (!depth_mm || !rgb || !pose) return refuse("a NULL image or pose");
  if (w != k->key_w || h != k->key_h) return refuse("the images do not have the store's size");
  const float own[4] = {k->cfg.fx, k->cfg.fy, k->cfg.cx, k->cfg.cy};
  if (!intr) intr = own;
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(pose[i])) return refuse("a pose entry is not finite");
  if (!(std::isfinite(intr[0]) && intr[0] > 0.0f && std::isfinite(intr[1]) && intr[1] > 0.0f && std::isfinite(intr[2]) && std::isfinite(intr[3])))
    return refuse("fx and fy must be finite and positive, cx and cy finite");
  if (k->key_n >= k->key_cap) return fail(k, HSK_ERR_STATE, "hsk_add_keyframe: the store is full");
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  // the slot as it lies in the store: record, colour words, depth
  const size_t px = (size_t)w * (size_t)h, bytes = 64 + 6 * px;
  std::vector<unsigned char> blob(bytes);
  KeyRecord rec;
  pose16_to_rt(pose, rec.R, rec.t);
  rec.fx = intr[0], rec.fy = intr[1], rec.cx = intr[2], rec.cy = intr[3];
  memcpy(blob.data(), &rec, 64);
  unsigned* cw = (unsigned*)(blob.data() + 64);
  for (size_t i = 0; i < px; ++i) cw[i] = (unsigned)rgb[3 * i] | ((unsigned)rgb[3 * i + 1] << 8) | ((unsigned)rgb[3 * i + 2] << 16);
  memcpy(blob.data() + 64 + 4 * px, depth_mm, 2 * px);
  // (the blob is pageable: the copy has left it when hipMemcpyAsync returns)
  HIPCHK(k, hipMemcpyAsync((char*)k->d_key + (size_t)k->key_n * key_slot_bytes(w, h), blob.data(), bytes, hipMemcpyHostToDevice, k->stream));
  float m[16];
  rt_to_pose16(rec.R, rec.t, m);
  k->key_rec.insert(k->key_rec.end(), m, m + 12);
  k->key_rec.insert(k->key_rec.end(), intr, intr + 4);
  if (index) *index = k->key_n;
  k->key_n += 1;
  return HSK_OK;
}

extern "C" int hsk_keyframe_count(const hsk_ctx* k, int* n, int* cap, int* w, int* h, uint64_t* bytes) {
  if (!k) return HSK_ERR_ARG;
  if (n) *n = k->key_n;
  if (cap) *cap = k->key_cap;
  if (w) *w = k->key_w;
  if (h) *h = k->key_h;
  if (bytes) *bytes = k->d_key ? (uint64_t)k->key_cap * (uint64_t)key_slot_bytes(k->key_w, k->key_h) : 0;
  return HSK_OK;
}

extern "C" int hsk_get_keyframe(hsk_ctx* k, int index, float pose[16], float intr[4], uint16_t* depth_mm, uint8_t* rgb) {
  if (!k) return HSK_ERR_ARG;
  if (!k->d_key) return fail(k, HSK_ERR_STATE, "hsk_get_keyframe: there is no keyframe store (hsk_enable_keyframes)");
  if (index < 0 || index >= k->key_n) return fail(k, HSK_ERR_ARG, "hsk_get_keyframe: the index lies outside 0 .. n - 1");
  const float* r = k->key_rec.data() + 16 * (size_t)index;
  if (pose) {
    memcpy(pose, r, 48);
    pose[12] = pose[13] = pose[14] = 0.0f;
    pose[15] = 1.0f;
  }
  if (intr) memcpy(intr, r + 12, 16);
  if (!depth_mm && !rgb) return HSK_OK;
  HIPCHK(k, hipSetDevice(k->cfg.device_id));
  const size_t px = (size_t)k->key_w * (size_t)k->key_h;
  const char* slot = (const char*)k->d_key + (size_t)index * key_slot_bytes(k->key_w, k->key_h);
  if (depth_mm)
    if (int rc = copy_out(k, depth_mm, slot + 64 + 4 * px, 2 * px)) return rc;
  if (rgb) {
    std::vector<unsigned> cw(px);
    if (int rc = copy_out(k, cw.data(), slot + 64, 4 * px)) return rc;
    for (size_t i = 0; i < px; ++i) {
      rgb[3 * i] = (uint8_t)(cw[i] & 255u);
      rgb[3 * i + 1] = (uint8_t)((cw[i] >> 8) & 255u);
      rgb[3 * i + 2] = (uint8_t)((cw[i] >> 16) & 255u);
    }
  }
  return HSK_OK;
}

extern "C" int hsk_clear_keyframes(hsk_ctx* k) {
  if (!k) return HSK_ERR_ARG;
  k->key_n = 0;  // (every bake has its results before it returns: nothing enqueued still reads the slots)
  k->key_rec.clear();
  return HSK_OK;
}

extern "C" int hsk_release_keyframes(hsk_ctx* k) {
  if (!k) return HSK_ERR_ARG;
  if (k->d_key) {
    HIPCHK(k, hipSetDevice(k->cfg.device_id));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    HIPCHK(k, hipFree(k->d_key));
    k->d_key = nullptr;
  }
  k->key_cap = k->key_w = k->key_h = k->key_n = 0;
  k->key_rec.clear();
  return HSK_OK;
}

extern "C" int hsk_keyframe_wanted(const float* poses, size_t n, const float pose[16], float min_translation_m, float min_angle_rad) {
  if (!pose || (n && !poses) || !(std::isfinite(min_translation_m) && min_translation_m >= 0.0f) ||
      !(std::isfinite(min_angle_rad) && min_angle_rad >= 0.0f))
    return HSK_ERR_ARG;
  for (size_t i = 0; i < n; ++i) {
    const float* p = poses + 16 * i;
    const double dx = (double)pose[3] - (double)p[3], dy = (double)pose[7] - (double)p[7], dz = (double)pose[11] - (double)p[11];
    const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
    double tr = 0.0;  // trace(Ri^T R): the sum of the products of like entries, row by row
    for (int r = 0; r < 3; ++r) tr += ((double)p[4 * r] * (double)pose[4 * r] + (double)p[4 * r + 1] * (double)pose[4 * r + 1]) + (double)p[4 * r + 2] * (double)pose[4 * r + 2];
    double c = (tr - 1.0) * 0.5;
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
    if (!(dist > (double)min_translation_m || acos(c) > (double)min_angle_rad)) return 0;
  }
  return 1;
}

extern "C" void hsk_default_keytex_params(const hsk_ctx* k, hsk_keytex_params* p) {
  if (!p) return;
  p->mode = HSK_KEYTEX_BEST;
  p->z_min_m = 0.3f;
  p->z_max_m = 4.0f;
  p->cos_min = 0.2f;
  p->border_px = 4.0f;
  p->occlusion_tol_m = k ? 3.0f * fmaxf(k->vp.cell[0], fmaxf(k->vp.cell[1], k->vp.cell[2])) : 0.03f;
  p->blend_floor = 0.5f;
  p->fallback_volume = 1;
}

extern "C" int hsk_bake_texture_keyframes(hsk_ctx* k, const float* vertices, size_t n_vertices, const int32_t* faces, size_t n_faces,
                                          const hsk_texture_params* tp, const hsk_keytex_params* kp, uint8_t* rgb, uint8_t* normal_rgb, uint8_t* mask,
                                          uint8_t* source, size_t cap_texels, float* uv, hsk_texture_chart* charts, hsk_texture_info* info,
                                          hsk_keytex_info* kinfo) {
  static_assert(sizeof(hsk_keytex_params) == 32 && sizeof(hsk_keytex_info) == 48, "the keyframe textures' structs");
  static_assert(TEX_KEYFRAME == HSK_TEXEL_KEYFRAME && KEY_BEST == HSK_KEYTEX_BEST && KEY_BLEND == HSK_KEYTEX_BLEND && KEY_NONE == HSK_KEYTEX_NONE,
                "the rule's constants are the ABI's");
  if (!k) return HSK_ERR_ARG;
  auto refuse = [&](const char* why) { return fail(k, HSK_ERR_ARG, (std::string("hsk_bake_texture_keyframes: ") + why).c_str()); };
  hsk_keytex_params p;
  hsk_default_keytex_params(k, &p);
  if (kp) p = *kp;
  if (p.mode != HSK_KEYTEX_BEST && p.mode != HSK_KEYTEX_BLEND) return refuse("mode must be HSK_KEYTEX_BEST or HSK_KEYTEX_BLEND");
  for (float f : {p.z_min_m, p.z_max_m, p.cos_min, p.border_px, p.occlusion_tol_m, p.blend_floor})
    if (!(std::isfinite(f) && f >= 0.0f)) return refuse("a parameter is negative or not finite");
  if (p.z_min_m > p.z_max_m) return refuse("z_min_m lies above z_max_m");
  if (p.cos_min > 1.0f) return refuse("cos_min lies above 1");
  if (p.blend_floor > 1.0f) return refuse("blend_floor lies outside [0, 1]");
  if (int rs = keytex_state(k, "hsk_bake_texture_keyframes", true)) return rs;
  KeyStore ks;
  ks.base = (const unsigned char*)k->d_key;
  ks.stride = key_slot_bytes(k->key_w, k->key_h);
  ks.n = k->key_n, ks.w = k->key_w, ks.h = k->key_h;
  KeyArgs ka;
  ka.mode = p.mode;
  ka.z_min = p.z_min_m, ka.z_max = p.z_max_m, ka.cos_min = p.cos_min, ka.border = p.border_px, ka.occlusion_tol = p.occlusion_tol_m;
  ka.blend_floor = p.blend_floor;
  ka.fallback = p.fallback_volume != 0;
  const KeyBake kb = {&ks, &ka, source, kinfo};
  return texture_bake(k, "hsk_bake_texture_keyframes", vertices, n_vertices, faces, n_faces, tp, rgb, normal_rgb, mask, cap_texels, uv, charts, info, &kb);
}
