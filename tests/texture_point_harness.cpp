// texture_point_harness.cpp -- housescan_amd/csrc/hsk_texture_point.h (the layout the ABI runs on the host and the text every lane
// of texture.hip's kernel runs) compiled for the host: lays one mesh out and bakes every texel of its atlas sequentially, for
// tests/test_texture_host.py to compare with the numpy twin.  Built with the address and undefined-behaviour sanitizers; a program
// of its own, nothing preloaded.
//   in : int32 X Y Z has_colour n_vertices n_faces W n_iter; float size[3], texels_per_metre, f_tol, max_offset_m; the vertices
//        (3 floats each), the faces (3 int32 each); the volume's pair words in the device's block layout; with colour X Y Z
//        (r, g, b, w) words, row-major
//   out: uint64 info[13] (hsk_texture_info); when info[1] <= 16384: the charts (4 int32 a face), uv (6 floats a face), rgb and
//        normal_rgb (3 W H bytes each), mask (W H bytes), the final points (3 W H floats)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../housescan_amd/csrc/hsk_texture_point.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hd[8];
  float fl[6];
  if (fread(hd, 4, 8, f) != 8 || fread(fl, 4, 6, f) != 6) return 2;
  SampleVol v;
  v.X = hd[0], v.Y = hd[1], v.Z = hd[2];
  const bool colour = hd[3] != 0;
  const size_t nv = (size_t)hd[4], nf = (size_t)hd[5];
  if (v.X < 4 || v.Y < 2 || v.Z < 2 || (v.X & 3) || hd[4] < 0 || hd[5] < 0) return 2;
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
  fclose(f);
  if (!ok) return 2;
  TexLayout L;
  std::vector<float> uv(6 * nf);
  tex_layout(verts.data(), nv, faces.data(), nf, (double)fl[3], hd[6], L, uv.data());
  unsigned long long info[13] = {(unsigned long long)L.W, (unsigned long long)L.H, L.n_charted, L.n_skipped, L.n_blocks[0], L.n_blocks[1],
                                 L.n_blocks[2], L.n_blocks[3], 0, 0, 0, 0, 0};
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  if (L.H > TEX_MAX_SIDE) {
    fwrite(info, 8, 13, o);
    return fclose(o) == 0 ? 0 : 2;
  }
  TexArgs ta;
  ta.W = (int)L.W;
  ta.H = (int)L.H;
  ta.n_iter = hd[7];
  ta.f_tol = fl[4];
  ta.max_offset2 = fl[5] * fl[5];
  const size_t texels = (size_t)ta.W * ta.H;
  std::vector<unsigned char> rgb(3 * texels), nrm(3 * texels), mask(texels);
  std::vector<float> pts(3 * texels);
  for (int py = 0; py < ta.H; ++py)
    for (int px = 0; px < ta.W; ++px) {
      TexelOut t;
      tex_texel(vol.data(), colour ? col.data() : nullptr, v, ta, L.tiles.data(), L.blocks.data(), faces.data(), verts.data(), px, py, t);
      const size_t i = (size_t)py * ta.W + px;
      for (int c = 0; c < 3; ++c) {
        rgb[3 * i + c] = (unsigned char)t.rgb[c];
        nrm[3 * i + c] = (unsigned char)t.nrm[c];
        pts[3 * i + c] = t.p[c];
      }
      mask[i] = (unsigned char)t.mask;
      for (int b = 0; b < 5; ++b) info[8 + b] += (t.mask >> b) & 1u;
    }
  fwrite(info, 8, 13, o);
  auto put = [&](const void* data, size_t bytes) {  // (an empty vector has no data to point at)
    if (bytes) fwrite(data, 1, bytes, o);
  };
  put(L.charts.data(), L.charts.size() * sizeof(TexChart));
  put(uv.data(), uv.size() * 4);
  put(rgb.data(), rgb.size());
  put(nrm.data(), nrm.size());
  put(mask.data(), mask.size());
  put(pts.data(), pts.size() * 4);
  return fclose(o) == 0 ? 0 : 2;
}
