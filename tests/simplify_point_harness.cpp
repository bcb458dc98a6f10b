// simplify_point_harness.cpp -- housescan_amd/csrc/hsk_simplify_point.h (the text the kernels of simplify.hip run) compiled for
// the host: simplifies one small volume sequentially, cluster by cluster as the gather kernel does -- the vertices from the c^3
// voxels of the cell, the triangles from the (c + 1)^3 cubes from one below it -- and writes every sum, vertex, normal, colour,
// face and the statistics for tests/test_simplify_host.py to compare with the numpy twin.  Built with the address and
// undefined-behaviour sanitizers; a program of its own, nothing preloaded.
//   in : int32 X Y Z c mode has_colour; float sv_floor, cell[3]; the marching-cubes table (256 counts, 256 x 5 x 3 edge codes);
//        X Y Z pair words (tsdf | weight << 16), row-major, x fastest; with colour as many (r, g, b, w) words
//   out: uint64 n_out n_faces; uint32 clusters[n_out]; int64 sums[n_out][20]; float vertices[n_out][3], normals[n_out][3];
//        uint8 rgb[n_out][3]; int32 faces[n_faces][3]; uint64 stats[12]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../housescan_amd/csrc/hsk_simplify_point.h"

struct Table {
  unsigned char ntri[256];
  unsigned char edge[256][5][3];
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hd[6];
  float fl[4];
  Table ct;
  if (fread(hd, 4, 6, f) != 6 || fread(fl, 4, 4, f) != 4 || fread(ct.ntri, 1, 256, f) != 256 || fread(ct.edge, 1, 256 * 15, f) != 256 * 15) return 2;
  const int X = hd[0], Y = hd[1], Z = hd[2], c = hd[3], mode = hd[4];
  const bool colour = hd[5] != 0;
  const int s = simp_shift(c);
  if (s < 0 || X < 2 || Y < 2 || Z < 2) return 2;
  const size_t nvox = (size_t)X * Y * Z;
  std::vector<unsigned> W(nvox), Cw(colour ? nvox : 0);
  if (fread(W.data(), 4, nvox, f) != nvox || (colour && fread(Cw.data(), 4, nvox, f) != nvox)) return 2;
  fclose(f);
  auto at = [&](int x, int y, int z) { return ((size_t)z * Y + y) * X + x; };
  auto cube = [&](int x, int y, int z, unsigned* w) {
    for (int k = 0; k < 8; ++k) w[k] = W[at(x + (k & 1), y + ((k >> 1) & 1), z + (k >> 2))];
  };
  const int CX = (X + c - 1) >> s, CY = (Y + c - 1) >> s, CZ = (Z + c - 1) >> s;
  const size_t ncl = (size_t)CX * CY * CZ;
  // the indexed mesh's edge bits: an edge has a vertex when it is cut and lies on a valid, cut cube
  std::vector<unsigned char> E(nvox, 0), ref(ncl, 0), touched(ncl, 0);
  unsigned long long n_in_faces = 0, n_in_vertices = 0;
  for (int z = 0; z < Z - 1; ++z)
    for (int y = 0; y < Y - 1; ++y)
      for (int x = 0; x < X - 1; ++x) {
        unsigned w[8];
        cube(x, y, z, w);
        const unsigned m8 = simp_m8(w);
        if (!m8) continue;
        n_in_faces += ct.ntri[m8];
        for (int a = 0; a < 8; ++a)
          for (int axis = 0; axis < 3; ++axis) {
            const int b = a | (1 << axis);
            if (b != a && (((m8 >> a) ^ (m8 >> b)) & 1u)) E[at(x + (a & 1), y + ((a >> 1) & 1), z + (a >> 2))] |= (unsigned char)(1u << axis);
          }
      }
  for (int z = 0; z < Z; ++z)
    for (int y = 0; y < Y; ++y)
      for (int x = 0; x < X; ++x) {
        const unsigned e = E[at(x, y, z)];
        if (!e) continue;
        n_in_vertices += (e & 1u) + ((e >> 1) & 1u) + ((e >> 2) & 1u);
        touched[((size_t)(z >> s) * CY + (y >> s)) * CX + (x >> s)] = 1;
      }
  // the surviving faces, in the indexed mesh's order, by their clusters' numbers
  std::vector<unsigned> face_ids;
  for (int z = 0; z < Z - 1; ++z)
    for (int y = 0; y < Y - 1; ++y)
      for (int x = 0; x < X - 1; ++x) {
        unsigned w[8];
        cube(x, y, z, w);
        const unsigned m8 = simp_m8(w);
        for (int t = 0; m8 && t < ct.ntri[m8]; ++t) {
          unsigned ids[3];
          if (!simp_face_clusters(ct.edge[m8][t], x, y, z, s, CX, CY, ids)) continue;
          for (int q = 0; q < 3; ++q) face_ids.push_back(ids[q]), ref[ids[q]] = 1;
        }
      }
  std::vector<unsigned> clusters;
  std::vector<int> number(ncl, -1);
  unsigned long long n_touched = 0;
  for (size_t id = 0; id < ncl; ++id) {
    n_touched += touched[id];
    if (ref[id]) number[id] = (int)clusters.size(), clusters.push_back((unsigned)id);
  }
  const size_t n_out = clusters.size(), n_faces = face_ids.size() / 3;
  std::vector<long long> sums(n_out * SIMP_REC, 0);
  std::vector<float> verts(n_out * 3), normals(n_out * 3);
  std::vector<unsigned char> rgb(n_out * 3, 0);
  unsigned long long stats[12] = {n_in_vertices, n_in_faces, n_touched, n_out, n_faces, n_in_faces - n_faces, 0, 0, 0, 0, 0, 0};
  const float cell[3] = {fl[1], fl[2], fl[3]};
  for (size_t j = 0; j < n_out; ++j) {
    const unsigned id = clusters[j];
    const int cl[3] = {(int)(id % (unsigned)CX), (int)((id / (unsigned)CX) % (unsigned)CY), (int)(id / (unsigned)(CX * CY))};
    const int base[3] = {cl[0] << s, cl[1] << s, cl[2] << s};
    simp_i64* rec = &sums[j * SIMP_REC];
    for (int i = 0; i < c * c * c; ++i) {
      const int g[3] = {base[0] + (i & (c - 1)), base[1] + ((i >> s) & (c - 1)), base[2] + (i >> (2 * s))};
      if (g[0] >= X || g[1] >= Y || g[2] >= Z) continue;
      const unsigned b3 = E[at(g[0], g[1], g[2])];
      const int fa = hsk_pair_raw(W[at(g[0], g[1], g[2])]);
      for (int k = 0; k < 3; ++k) {
        if (!((b3 >> k) & 1u)) continue;
        const int h[3] = {g[0] + (k == 0), g[1] + (k == 1), g[2] + (k == 2)};
        const int fb = hsk_pair_raw(W[at(h[0], h[1], h[2])]);
        simp_i64 p[3];
        simp_position(g, k, fa, fb, base, c, p);
        simp_add_vertex(rec, p, colour ? simp_color_pick(fa, fb, Cw[at(g[0], g[1], g[2])], Cw[at(h[0], h[1], h[2])]) : 0u);
      }
    }
    const int n1 = c + 1;
    for (int i = 0; i < n1 * n1 * n1; ++i) {
      const int dz = i / (n1 * n1), r = i - dz * n1 * n1, dy = r / n1, dx = r - dy * n1;
      const int x = base[0] - 1 + dx, y = base[1] - 1 + dy, z = base[2] - 1 + dz;
      if (x < 0 || y < 0 || z < 0 || x >= X - 1 || y >= Y - 1 || z >= Z - 1) continue;
      unsigned w[8];
      cube(x, y, z, w);
      const unsigned m8 = simp_m8(w);
      if (m8) simp_cube_triangles(ct, w, m8, x, y, z, s, cl, rec);
    }
    double xq[3];
    int rank, clamped;
    simp_vertex(rec, c, mode, (double)fl[0], xq, &rank, &clamped);
    stats[6 + rank] += 1;
    stats[10] += (unsigned long long)clamped;
    simp_metres(xq, c, cl, cell, &verts[3 * j]);
    if (!simp_normal(rec, cell, &normals[3 * j])) normals[3 * j] = normals[3 * j + 1] = normals[3 * j + 2] = __builtin_nanf("");
    if (colour && !simp_rgb(rec, &rgb[3 * j])) stats[11] += 1;
  }
  std::vector<int> faces(face_ids.size());
  for (size_t i = 0; i < face_ids.size(); ++i) faces[i] = number[face_ids[i]];
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const unsigned long long head[2] = {n_out, n_faces};
  fwrite(head, 8, 2, o);
  auto put = [&](const void* data, size_t bytes) {  // (an empty vector has no data to point at)
    if (bytes) fwrite(data, 1, bytes, o);
  };
  put(clusters.data(), n_out * 4);
  put(sums.data(), sums.size() * 8);
  put(verts.data(), verts.size() * 4);
  put(normals.data(), normals.size() * 4);
  put(rgb.data(), rgb.size());
  put(faces.data(), faces.size() * 4);
  fwrite(stats, 8, 12, o);
  return fclose(o) == 0 ? 0 : 2;
}
