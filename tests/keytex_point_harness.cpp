// keytex_point_harness.cpp -- housescan_amd/csrc/hsk_keytex_point.h (the text every lane of keytex.hip's kernel runs, over
// hsk_texture_point.h) compiled for the host: lays one mesh out, packs the keyframes into a store as hsk_add_keyframe does and bakes
// every texel of the atlas sequentially, for tests/test_keytex_host.py to compare with the numpy twin.  Built with the address and
// undefined-behaviour sanitizers; a program of its own, nothing preloaded.
//   in : int32 X Y Z has_colour n_vertices n_faces W n_iter n_keyframes kw kh mode fallback; float size[3], texels_per_metre, f_tol,
//        max_offset_m, z_min, z_max, cos_min, border, occlusion_tol, blend_floor; the vertices (3 floats each), the faces (3 int32
//        each); the volume's pair words in the device's block layout; with colour X Y Z (r, g, b, w) words, row-major; per keyframe
//        16 floats (R row-major, t, fx fy cx cy), kw kh rgb triples, kw kh uint16 depths
//   out: uint64 info[13] (hsk_texture_info), kinfo[6] (hsk_keytex_info); the charts (4 int32 a face), uv (6 floats a face), rgb and
//        normal_rgb (3 W H bytes each), mask and source (W H bytes each), the final points (3 W H floats)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../housescan_amd/csrc/hsk_keytex_point.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hd[13];
  float fl[12];
  if (fread(hd, 4, 13, f) != 13 || fread(fl, 4, 12, f) != 12) return 2;
  SampleVol v;
  v.X = hd[0], v.Y = hd[1], v.Z = hd[2];
  const bool colour = hd[3] != 0;
  const size_t nv = (size_t)hd[4], nf = (size_t)hd[5];
  const int nk = hd[8], kw = hd[9], kh = hd[10];
  if (v.X < 4 || v.Y < 2 || v.Z < 2 || (v.X & 3) || hd[4] < 0 || hd[5] < 0 || nk < 0 || nk > KEY_MAX_CAP || kw < 2 || kh < 2 || kw > KEY_MAX_SIDE ||
      kh > KEY_MAX_SIDE)
    return 2;
  const int dims[3] = {v.X, v.Y, v.Z};
  for (int i = 0; i < 3; ++i) {
    v.cell[i] = fl[i] / (float)dims[i];
    v.icell[i] = 1.0 / (double)v.cell[i];
  }
  std::vector<float> verts(3 * nv);
  std::vector<int32_t> faces(3 * nf);
  const size_t nvox = (size_t)v.X * v.Y * v.Z, nwords = (size_t)v.X * v.Y * ((v.Z + 3) & ~3);
  std::vector<unsigned> vol(nwords), col(colour ? nvox : 0);
  bool ok = (!nv || fread(verts.data(), 12, nv, f) == nv) && (!nf || fread(faces.data(), 12, nf, f) == nf) &&
            fread(vol.data(), 4, nwords, f) == nwords && (!colour || fread(col.data(), 4, nvox, f) == nvox);
  // the store as hsk_add_keyframe writes it, slot by slot; the allocation ends with the last slot's images, so a tap past them is
  // the sanitizer's (words: the records and the colour images are aligned)
  const size_t px = (size_t)kw * kh, stride = key_slot_bytes(kw, kh);
  std::vector<unsigned> store(nk ? ((size_t)(nk - 1) * stride + 64 + 6 * px + 3) / 4 : 0, 0u);
  std::vector<unsigned char> rgb_in(3 * px);
  for (int k = 0; ok && k < nk; ++k) {
    unsigned char* s = (unsigned char*)store.data() + (size_t)k * stride;
    ok = fread(s, 4, 16, f) == 16 && fread(rgb_in.data(), 3, px, f) == px && fread(s + 64 + 4 * px, 2, px, f) == px;
    unsigned* cw = (unsigned*)(s + 64);
    for (size_t i = 0; i < px; ++i) cw[i] = (unsigned)rgb_in[3 * i] | ((unsigned)rgb_in[3 * i + 1] << 8) | ((unsigned)rgb_in[3 * i + 2] << 16);
  }
  KeyStore ks;
  ks.base = (const unsigned char*)store.data();
  ks.stride = stride;
  ks.n = nk, ks.w = kw, ks.h = kh;
  fclose(f);
  if (!ok) return 2;
  TexLayout L;
  std::vector<float> uv(6 * nf);
  tex_layout(verts.data(), nv, faces.data(), nf, (double)fl[3], hd[6], L, uv.data());
  unsigned long long info[13] = {(unsigned long long)L.W, (unsigned long long)L.H, L.n_charted, L.n_skipped, L.n_blocks[0], L.n_blocks[1],
                                 L.n_blocks[2], L.n_blocks[3], 0, 0, 0, 0, 0};
  unsigned long long kinfo[6] = {(unsigned long long)nk, 0, 0, 0, 0, 0};
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  if (L.H > TEX_MAX_SIDE) return 2;
  TexArgs ta;
  ta.W = (int)L.W;
  ta.H = (int)L.H;
  ta.n_iter = hd[7];
  ta.f_tol = fl[4];
  ta.max_offset2 = fl[5] * fl[5];
  KeyArgs ka;
  ka.mode = hd[11];
  ka.fallback = hd[12];
  ka.z_min = fl[6], ka.z_max = fl[7], ka.cos_min = fl[8], ka.border = fl[9], ka.occlusion_tol = fl[10], ka.blend_floor = fl[11];
  const size_t texels = (size_t)ta.W * ta.H;
  std::vector<unsigned char> rgb(3 * texels), nrm(3 * texels), mask(texels), source(texels);
  std::vector<float> pts(3 * texels);
  for (int py = 0; py < ta.H; ++py)
    for (int px_ = 0; px_ < ta.W; ++px_) {
      KeyTexelOut t;
      key_texel(vol.data(), colour ? col.data() : nullptr, v, ta, L.tiles.data(), L.blocks.data(), faces.data(), verts.data(), ks, ka, px_, py,
                KeyAnyOne(), t);
      const size_t i = (size_t)py * ta.W + px_;
      for (int c = 0; c < 3; ++c) {
        rgb[3 * i + c] = (unsigned char)t.rgb[c];
        nrm[3 * i + c] = (unsigned char)t.nrm[c];
        pts[3 * i + c] = t.p[c];
      }
      mask[i] = (unsigned char)t.mask;
      source[i] = (unsigned char)t.source;
      for (int b = 0; b < 5; ++b) info[8 + b] += (t.mask >> b) & 1u;
      kinfo[1] += (t.mask >> 5) & 1u;
      kinfo[2] += (t.mask >> 3) & 1u;
      kinfo[3] += (t.mask & 1u) && !(t.mask & (TEX_KEYFRAME | TEX_COLORED));
      kinfo[4] += t.seen;
      kinfo[5] += t.occluded;
    }
  fwrite(info, 8, 13, o);
  fwrite(kinfo, 8, 6, o);
  auto put = [&](const void* data, size_t bytes) {  // (an empty vector has no data to point at)
    if (bytes) fwrite(data, 1, bytes, o);
  };
  put(L.charts.data(), L.charts.size() * sizeof(TexChart));
  put(uv.data(), uv.size() * 4);
  put(rgb.data(), rgb.size());
  put(nrm.data(), nrm.size());
  put(mask.data(), mask.size());
  put(source.data(), source.size());
  put(pts.data(), pts.size() * 4);
  return fclose(o) == 0 ? 0 : 2;
}
