// api_texture.hip -- the C ABI's baked textures (include/hskinfu.h "Baked textures"; DESIGN.md 3.25 the kernel, 8s the rule):
// hsk_default_texture_params, hsk_texture_layout (the layout alone, host only) and hsk_bake_texture.  The layout runs on the host
// inside the call (hsk_texture_point.h: tex_layout, the text the host harness runs); the mesh, the block records and the tile
// table go up in one copy into the product buffer, the kernel bakes into the same buffer and the images come back through the
// pinned pair.  It reads the volume as it stands, with no flush of the deferred weights -- the rule asks of a weight only whether
// it is zero (hsk_sample_min_weight), as the alignment does --, and writes nothing but the product buffer.  texture_bake is that
// path for both bakes: hsk_bake_texture_keyframes (api_keytex.hip) passes its store and gets the source plane and its counts.
#pragma clang fp contract(off)
#include <cmath>

#include "hsk_ctx.h"
#include "hsk_keytex_point.h"

extern "C" void hsk_default_texture_params(const hsk_ctx* k, hsk_texture_params* p) {
  (void)k;  // (the defaults that depend on the volume are the zeros: hsk_bake_texture resolves them)
  if (!p) return;
  p->texels_per_metre = 0.0f;
  p->atlas_width = 0;
  p->n_iter = 4;
  p->f_tol = 0.01f;
  p->max_offset_m = 0.0f;
}

static const char* texture_width(int* w) {
  if (*w == 0) *w = 1024;
  if (*w < 64 || *w > TEX_MAX_SIDE || (*w & 63)) return "atlas_width is no multiple of 64 in 64 .. 16384 (0: the default, 1024)";
  return nullptr;
}

static void texture_info(const TexLayout& L, hsk_texture_info* info) {
  if (!info) return;
  memset(info, 0, sizeof(*info));
  info->width = (uint64_t)L.W;
  info->height = (uint64_t)L.H;
  info->n_faces_charted = L.n_charted;
  info->n_faces_skipped = L.n_skipped;
  for (int i = 0; i < 4; ++i) info->n_blocks[i] = L.n_blocks[i];
}

// the mesh as a layout takes it, or the message
static const char* texture_mesh(const float* vertices, size_t n_vertices, const int32_t* faces, size_t n_faces) {
  if ((n_vertices && !vertices) || (n_faces && !faces)) return "a NULL mesh array with a count above 0";
  if (n_vertices > (size_t)INT32_MAX || n_faces > (size_t)INT32_MAX) return "more than INT32_MAX vertices or faces";
  return nullptr;
}

static void texture_charts(const TexLayout& L, hsk_texture_chart* charts) {
  static_assert(sizeof(hsk_texture_chart) == sizeof(TexChart) && sizeof(hsk_texture_chart) == 16, "a chart record is 16 bytes");
  if (charts && !L.charts.empty()) memcpy(charts, L.charts.data(), L.charts.size() * sizeof(TexChart));
}

extern "C" int hsk_texture_layout(const float* vertices, size_t n_vertices, const int32_t* faces, size_t n_faces, float texels_per_metre,
                                  int atlas_width, float* uv, hsk_texture_chart* charts, hsk_texture_info* info) {
  auto refuse = [](const char* why) {
    create_error() = std::string("hsk_texture_layout: ") + why;
    return HSK_ERR_ARG;
  };
  if (const char* why = texture_mesh(vertices, n_vertices, faces, n_faces)) return refuse(why);
  if (!(std::isfinite(texels_per_metre) && texels_per_metre > 0.0f)) return refuse("texels_per_metre must be finite and above 0");
  if (const char* why = texture_width(&atlas_width)) return refuse(why);
  TexLayout L;
  std::vector<float> uvs(uv ? 6 * n_faces : 0);  // (uv is written whole or not at all)
  tex_layout(vertices, n_vertices, faces, n_faces, (double)texels_per_metre, atlas_width, L, uv ? uvs.data() : nullptr);
  texture_info(L, info);
  if (L.H > TEX_MAX_SIDE) return refuse("the atlas would be higher than 16384 texels (info.height: lower texels_per_metre or widen the atlas)");
  if (uv && n_faces) memcpy(uv, uvs.data(), uvs.size() * 4);
  texture_charts(L, charts);
  return HSK_OK;
}

int texture_bake(hsk_ctx* k, const char* who, const float* vertices, size_t n_vertices, const int32_t* faces, size_t n_faces,
                 const hsk_texture_params* params, uint8_t* rgb, uint8_t* normal_rgb, uint8_t* mask, size_t cap_texels, float* uv,
                 hsk_texture_chart* charts, hsk_texture_info* info, const KeyBake* kb) {
  static_assert(sizeof(hsk_texture_params) == 20 && sizeof(hsk_texture_info) == 104, "the baked textures' structs");
  if (!k) return HSK_ERR_ARG;
  auto refuse = [&](const char* why) { return fail(k, HSK_ERR_ARG, (std::string(who) + ": " + why).c_str()); };
  uint8_t* source = kb ? kb->source : nullptr;
  if (const char* why = texture_mesh(vertices, n_vertices, faces, n_faces)) return refuse(why);
  hsk_texture_params p;
  hsk_default_texture_params(k, &p);
  if (params) p = *params;
  const float* cell = k->vp.cell;
  const float cmin = fminf(cell[0], fminf(cell[1], cell[2])), cmax = fmaxf(cell[0], fmaxf(cell[1], cell[2]));
  if (!(std::isfinite(p.texels_per_metre) && p.texels_per_metre >= 0.0f)) return refuse("texels_per_metre must be finite and not negative (0: one texel per voxel)");
  if (p.texels_per_metre == 0.0f) p.texels_per_metre = 1.0f / cmin;
  if (const char* why = texture_width(&p.atlas_width)) return refuse(why);
  if (p.n_iter < 0 || p.n_iter > TEX_MAX_ITER) return refuse("n_iter must lie in 0 .. 16");
  if (!(std::isfinite(p.f_tol) && p.f_tol >= 0.0f)) return refuse("f_tol must be finite and not negative");
  if (!(std::isfinite(p.max_offset_m) && p.max_offset_m >= 0.0f)) return refuse("max_offset_m must be finite and not negative (0: 4 x the largest cell)");
  if (p.max_offset_m == 0.0f) p.max_offset_m = 4.0f * cmax;
  if (int rs = require_whole_volume(k, k, who, "a texel's taps would straddle the slabs")) return rs;
  if (rgb && !kb && require_color(k)) return HSK_ERR_STATE;  // (a keyframe bake asks the colour volume only where there is one)
  TexLayout L;
  std::vector<float> uvs(uv ? 6 * n_faces : 0);
  tex_layout(vertices, n_vertices, faces, n_faces, (double)p.texels_per_metre, p.atlas_width, L, uv ? uvs.data() : nullptr);
  hsk_texture_info in;
  texture_info(L, &in);
  if (info) *info = in;
  if (L.H > TEX_MAX_SIDE) return refuse("the atlas would be higher than 16384 texels (info.height: lower texels_per_metre or widen the atlas)");
  const size_t texels = (size_t)L.W * (size_t)L.H;
  const bool bake = rgb || normal_rgb || mask || source;
  hsk_keytex_info kin;
  memset(&kin, 0, sizeof(kin));
  if (kb) kin.n_keyframes = (uint64_t)kb->ks->n;
  if (kb && kb->kinfo) *kb->kinfo = kin;
  if (bake && cap_texels < texels) return refuse("cap_texels below width x height (the images are written whole or not at all)");
  if (bake && texels) {
    HIPCHK(k, hipSetDevice(k->cfg.device_id));
    // one blob up: vertices, faces, block records, tile table (each 256-byte aligned, as they lie in the product buffer)
    ProductLayout lay;
    const size_t v_at = lay.take(n_vertices * 12), f_at = lay.take(n_faces * 12), b_at = lay.take(L.blocks.size() * sizeof(TexBlock)),
                 t_at = lay.take(L.tiles.size() * 4);
    const size_t up_bytes = lay.bytes;
    const size_t c_at = lay.take((size_t)HSK_VIEW_COUNT_SLOTS * 16 * 8);
    const size_t rgb_at = lay.take(rgb ? 3 * texels : 0), nrm_at = lay.take(normal_rgb ? 3 * texels : 0), m_at = lay.take(mask ? texels : 0);
    const size_t s_at = lay.take(source ? texels : 0);
    int r = ensure_product_bytes(k, lay.bytes);
    if (r != HSK_OK) return r;
    std::vector<unsigned char> blob(up_bytes, 0);
    memcpy(blob.data() + v_at, vertices, n_vertices * 12);
    memcpy(blob.data() + f_at, faces, n_faces * 12);
    memcpy(blob.data() + b_at, L.blocks.data(), L.blocks.size() * sizeof(TexBlock));
    memcpy(blob.data() + t_at, L.tiles.data(), L.tiles.size() * 4);
    char* ob = (char*)k->d_out;
    HIPCHK(k, hipMemcpyAsync(ob, blob.data(), up_bytes, hipMemcpyHostToDevice, k->stream));
    HIPCHK(k, hipMemsetAsync(ob + c_at, 0, lay.bytes - c_at, k->stream));  // the counters and the images (an empty tile's wave writes nothing)
    if (source) HIPCHK(k, hipMemsetAsync(ob + s_at, KEY_NONE, texels, k->stream));
    TexArgs ta;
    ta.W = (int)L.W;
    ta.H = (int)L.H;
    ta.n_iter = p.n_iter;
    ta.f_tol = p.f_tol;
    ta.max_offset2 = p.max_offset_m * p.max_offset_m;
    if (kb)
      launch_bake_keytex(k->stream, k->d_vol, k->d_color, k->vp, ta, *kb->ks, *kb->ka, (const unsigned*)(ob + t_at), (const TexBlock*)(ob + b_at),
                         (const int*)(ob + f_at), (const float*)(ob + v_at), rgb ? (unsigned char*)(ob + rgb_at) : nullptr,
                         normal_rgb ? (unsigned char*)(ob + nrm_at) : nullptr, mask ? (unsigned char*)(ob + m_at) : nullptr,
                         source ? (unsigned char*)(ob + s_at) : nullptr, (unsigned long long*)(ob + c_at));
    else
      launch_bake_texture(k->stream, k->d_vol, k->d_color, k->vp, ta, (const unsigned*)(ob + t_at), (const TexBlock*)(ob + b_at),
                          (const int*)(ob + f_at), (const float*)(ob + v_at), rgb ? (unsigned char*)(ob + rgb_at) : nullptr,
                          normal_rgb ? (unsigned char*)(ob + nrm_at) : nullptr, mask ? (unsigned char*)(ob + m_at) : nullptr,
                          (unsigned long long*)(ob + c_at));
    HIPCHK(k, hipGetLastError());
    // (the blob is pageable: the copy has left it when hipMemcpyAsync returns)
    if (rgb) r = copy_out(k, rgb, ob + rgb_at, 3 * texels);
    if (r == HSK_OK && normal_rgb) r = copy_out(k, normal_rgb, ob + nrm_at, 3 * texels);
    if (r == HSK_OK && mask) r = copy_out(k, mask, ob + m_at, texels);
    if (r == HSK_OK && source) r = copy_out(k, source, ob + s_at, texels);
    if (r != HSK_OK) return r;
    unsigned long long slots[HSK_VIEW_COUNT_SLOTS * 16];
    r = copy_out(k, slots, ob + c_at, sizeof(slots));
    if (r != HSK_OK) return r;
    unsigned long long n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < HSK_VIEW_COUNT_SLOTS; ++s)
      for (int c = 0; c < 8; ++c) n[c] += slots[s * 16 + c];
    in.n_owned = n[0], in.n_inside = n[1], in.n_projected = n[2], in.n_colored = n[3], in.n_normal = n[4];
    if (info) *info = in;
    // (the colour volume colours a texel of a keyframe bake only as the fallback)
    kin.n_keyed = n[5], kin.n_fallback = n[3], kin.n_uncolored = n[0] - n[5] - n[3], kin.n_pairs_seen = n[6], kin.n_pairs_occluded = n[7];
    if (kb && kb->kinfo) *kb->kinfo = kin;
  }
  if (uv && n_faces) memcpy(uv, uvs.data(), uvs.size() * 4);
  texture_charts(L, charts);
  return HSK_OK;
}

extern "C" int hsk_bake_texture(hsk_ctx* k, const float* vertices, size_t n_vertices, const int32_t* faces, size_t n_faces,
                                const hsk_texture_params* params, uint8_t* rgb, uint8_t* normal_rgb, uint8_t* mask, size_t cap_texels, float* uv,
                                hsk_texture_chart* charts, hsk_texture_info* info) {
  return texture_bake(k, "hsk_bake_texture", vertices, n_vertices, faces, n_faces, params, rgb, normal_rgb, mask, cap_texels, uv, charts, info, nullptr);
}
