// harness_io.h -- the file handling the host harnesses (tests/*_harness.cpp) share: the input file argv[1] read piece by piece with
// one sticky status, the volume's size in words, and the output file argv[2] written the same way.  A harness returns 2 on any
// failure of either.  Nothing of housescan_amd/csrc is included here.
#pragma once
#include <cstddef>
#include <cstdio>
#include <vector>

struct HarnessIn {
  FILE* f;
  bool ok;
  // `files` is the number of file arguments the harness takes: 1 if it prints its result, 2 if it writes argv[2]
  HarnessIn(int argc, char** argv, int files) : f(argc > files ? fopen(argv[1], "rb") : nullptr), ok(f != nullptr) {}
  HarnessIn(const HarnessIn&) = delete;
  ~HarnessIn() {
    if (f) fclose(f);
  }
  template <class T>
  bool get(T* p, size_t count) {  // (no null pointer to fread: the data() of an empty vector may be one)
    ok = ok && (count == 0 || fread(p, sizeof(T), count, f) == count);
    return ok;
  }
  template <class T>
  bool get(std::vector<T>& v) {
    return get(v.data(), v.size());
  }
};

// (exactly the volume's words, as the device allocates them: an access past them is the sanitizer's to find)
inline size_t volume_words(size_t X, size_t Y, size_t Z) { return X * Y * ((Z + 3) & ~(size_t)3); }

// the device's table of labelled regions -- eight words a root: count, lo[3], hi[3], one unused -- from records indexed by root
template <class Rec>
std::vector<unsigned> region_table(const std::vector<Rec>& by_root, const std::vector<unsigned>& roots) {
  std::vector<unsigned> table(roots.size() * 8, 0u);
  for (size_t i = 0; i < roots.size(); ++i) {
    const Rec& c = by_root[roots[i]];
    table[i * 8] = (unsigned)c.n_voxels;
    for (int a = 0; a < 3; ++a) {
      table[i * 8 + 1 + a] = (unsigned)c.lo[a];
      table[i * 8 + 4 + a] = (unsigned)c.hi[a];
    }
  }
  return table;
}

struct HarnessOut {
  FILE* o;
  bool ok;
  explicit HarnessOut(const char* path) : o(fopen(path, "wb")), ok(o != nullptr) {}
  HarnessOut(const HarnessOut&) = delete;
  template <class T>
  void put(const T* p, size_t count) {
    ok = ok && (count == 0 || fwrite(p, sizeof(T), count, o) == count);
  }
  template <class T>
  void put(const std::vector<T>& v) {
    put(v.data(), v.size());
  }
  int finish() {  // -> the harness's exit status
    const bool closed = o && fclose(o) == 0;
    o = nullptr;
    return closed && ok ? 0 : 2;
  }
};
