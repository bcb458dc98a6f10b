// volume_image.cpp -- host side of the "HSKV" sparse volume image: header writer, validator.  No device code.
#include "hsk_volume_image.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

namespace {
template <class T>
T rd(const unsigned char* p, size_t at) {
  T v;
  memcpy(&v, p + at, sizeof(T));
  return v;
}
template <class T>
void wr(unsigned char* p, size_t at, T v) {
  memcpy(p + at, &v, sizeof(T));
}
int refuse(std::string* why, const char* msg) {
  if (why) *why = std::string("volume image: ") + msg;
  return HSK_ERR_ARG;
}
// one class table against the header: legal bytes, zero padding, the counts
int check_table(const unsigned char* tab, uint64_t n_bricks, uint64_t table_bytes, bool color, const uint64_t* want, std::string* why) {
  uint64_t n[4] = {0, 0, 0, 0};
  for (uint64_t i = 0; i < n_bricks; ++i) {
    const unsigned c = tab[i];
    if (c > 3u || (color && c != 0u && c != 3u)) return refuse(why, color ? "illegal colour class byte" : "illegal class byte");
    n[c] += 1;
  }
  for (uint64_t i = n_bricks; i < table_bytes; ++i)
    if (tab[i] != 0) return refuse(why, "class table padding is not zero");
  if (color ? (n[0] != want[0] || n[3] != want[1]) : (n[0] != want[0] || n[1] != want[1] || n[2] != want[2] || n[3] != want[3]))
    return refuse(why, "the header's brick counts and section lengths disagree with the class table");
  return HSK_OK;
}
}  // namespace

uint64_t hskv_bricks(const int32_t dims[3], int32_t nz) {
  return (uint64_t)(dims[0] >> 3) * (uint64_t)(dims[1] >> 3) * (uint64_t)((nz + 7) >> 3);
}
uint64_t hskv_table_bytes(uint64_t n_bricks) { return (n_bricks + 7) & ~(uint64_t)7; }

void hskv_finish_info(hsk_volume_info* info) {
  info->version = HSKV_VERSION;
  info->header_bytes = HSKV_HEADER_BYTES;
  info->n_bricks = hskv_bricks(info->dims, info->nz);
  info->tsdf_table_bytes = hskv_table_bytes(info->n_bricks);
  info->tsdf_payload_bytes =
      info->tsdf_bricks[1] * HSKV_REC_UNIFORM + info->tsdf_bricks[2] * HSKV_REC_SPLIT + info->tsdf_bricks[3] * HSKV_REC_RAW;
  if (info->flags & 1u) {
    info->color_table_bytes = info->tsdf_table_bytes;
    info->color_payload_bytes = info->color_bricks[1] * HSKV_REC_RAW;
  } else {
    info->color_bricks[0] = info->color_bricks[1] = 0;
    info->color_table_bytes = info->color_payload_bytes = 0;
  }
  info->total_bytes = HSKV_HEADER_BYTES + info->tsdf_table_bytes + info->tsdf_payload_bytes + info->color_table_bytes + info->color_payload_bytes;
}

void hskv_write_header(const hsk_volume_info* f, unsigned char out[HSKV_HEADER_BYTES]) {
  memset(out, 0, HSKV_HEADER_BYTES);
  memcpy(out + HSKV_AT_MAGIC, "HSKV", 4);
  wr<uint32_t>(out, HSKV_AT_VERSION, f->version);
  wr<uint32_t>(out, HSKV_AT_HEADER_BYTES, f->header_bytes);
  wr<uint32_t>(out, HSKV_AT_FLAGS, f->flags);
  for (int i = 0; i < 3; ++i) wr<int32_t>(out, HSKV_AT_DIMS + 4 * i, f->dims[i]);
  wr<int32_t>(out, HSKV_AT_Z0, f->z0);
  wr<int32_t>(out, HSKV_AT_NZ, f->nz);
  for (int i = 0; i < 3; ++i) wr<float>(out, HSKV_AT_SIZE_M + 4 * i, f->size_m[i]);
  wr<float>(out, HSKV_AT_TRUNC, f->trunc_dist_m);
  wr<float>(out, HSKV_AT_TRUNC_EFF, f->trunc_eff_m);
  wr<int32_t>(out, HSKV_AT_WIDTH, f->width);
  wr<int32_t>(out, HSKV_AT_HEIGHT, f->height);
  wr<float>(out, HSKV_AT_INTR, f->fx);
  wr<float>(out, HSKV_AT_INTR + 4, f->fy);
  wr<float>(out, HSKV_AT_INTR + 8, f->cx);
  wr<float>(out, HSKV_AT_INTR + 12, f->cy);
  for (int i = 0; i < 16; ++i) wr<float>(out, HSKV_AT_POSE + 4 * i, f->pose[i]);
  wr<int32_t>(out, HSKV_AT_FRAME, f->frame);
  wr<int32_t>(out, HSKV_AT_COLOR_MAXW, f->color_max_weight);
  wr<float>(out, HSKV_AT_COLOR_BAND, f->color_band_m);
  wr<uint64_t>(out, HSKV_AT_N_BRICKS, f->n_bricks);
  for (int i = 0; i < 4; ++i) wr<uint64_t>(out, HSKV_AT_TSDF_BRICKS + 8 * i, f->tsdf_bricks[i]);
  for (int i = 0; i < 2; ++i) wr<uint64_t>(out, HSKV_AT_COLOR_BRICKS + 8 * i, f->color_bricks[i]);
  wr<uint64_t>(out, HSKV_AT_TSDF_TABLE, f->tsdf_table_bytes);
  wr<uint64_t>(out, HSKV_AT_TSDF_PAYLOAD, f->tsdf_payload_bytes);
  wr<uint64_t>(out, HSKV_AT_COLOR_TABLE, f->color_table_bytes);
  wr<uint64_t>(out, HSKV_AT_COLOR_PAYLOAD, f->color_payload_bytes);
  wr<uint64_t>(out, HSKV_AT_TOTAL, f->total_bytes);
}

int hskv_parse_header(const void* buf, size_t n_bytes, hsk_volume_info* f, std::string* why) {
  if (n_bytes < HSKV_HEADER_BYTES) return refuse(why, "shorter than its header (256 bytes)");
  const unsigned char* p = (const unsigned char*)buf;
  if (memcmp(p + HSKV_AT_MAGIC, "HSKV", 4) != 0) return refuse(why, "bad magic (not an HSKV file)");
  memset(f, 0, sizeof(*f));
  f->version = rd<uint32_t>(p, HSKV_AT_VERSION);
  if (f->version != HSKV_VERSION) return refuse(why, "unsupported version (this library reads version 1)");
  f->header_bytes = rd<uint32_t>(p, HSKV_AT_HEADER_BYTES);
  if (f->header_bytes != HSKV_HEADER_BYTES) return refuse(why, "header size is not 256");
  f->flags = rd<uint32_t>(p, HSKV_AT_FLAGS);
  for (int i = 0; i < 3; ++i) f->dims[i] = rd<int32_t>(p, HSKV_AT_DIMS + 4 * i);
  f->z0 = rd<int32_t>(p, HSKV_AT_Z0);
  f->nz = rd<int32_t>(p, HSKV_AT_NZ);
  for (int i = 0; i < 3; ++i) f->size_m[i] = rd<float>(p, HSKV_AT_SIZE_M + 4 * i);
  f->trunc_dist_m = rd<float>(p, HSKV_AT_TRUNC);
  f->trunc_eff_m = rd<float>(p, HSKV_AT_TRUNC_EFF);
  f->width = rd<int32_t>(p, HSKV_AT_WIDTH);
  f->height = rd<int32_t>(p, HSKV_AT_HEIGHT);
  f->fx = rd<float>(p, HSKV_AT_INTR);
  f->fy = rd<float>(p, HSKV_AT_INTR + 4);
  f->cx = rd<float>(p, HSKV_AT_INTR + 8);
  f->cy = rd<float>(p, HSKV_AT_INTR + 12);
  for (int i = 0; i < 16; ++i) f->pose[i] = rd<float>(p, HSKV_AT_POSE + 4 * i);
  f->frame = rd<int32_t>(p, HSKV_AT_FRAME);
  f->color_max_weight = rd<int32_t>(p, HSKV_AT_COLOR_MAXW);
  f->color_band_m = rd<float>(p, HSKV_AT_COLOR_BAND);
  f->n_bricks = rd<uint64_t>(p, HSKV_AT_N_BRICKS);
  for (int i = 0; i < 4; ++i) f->tsdf_bricks[i] = rd<uint64_t>(p, HSKV_AT_TSDF_BRICKS + 8 * i);
  for (int i = 0; i < 2; ++i) f->color_bricks[i] = rd<uint64_t>(p, HSKV_AT_COLOR_BRICKS + 8 * i);
  f->tsdf_table_bytes = rd<uint64_t>(p, HSKV_AT_TSDF_TABLE);
  f->tsdf_payload_bytes = rd<uint64_t>(p, HSKV_AT_TSDF_PAYLOAD);
  f->color_table_bytes = rd<uint64_t>(p, HSKV_AT_COLOR_TABLE);
  f->color_payload_bytes = rd<uint64_t>(p, HSKV_AT_COLOR_PAYLOAD);
  f->total_bytes = rd<uint64_t>(p, HSKV_AT_TOTAL);
  // self-consistency
  if ((f->flags & ~1u) != 0u) return refuse(why, "unknown flag bits");
  for (int i = 0; i < 3; ++i) {
    if (f->dims[i] <= 0 || (i < 2 && (f->dims[i] & 7) != 0)) return refuse(why, "dims must be positive, x and y multiples of 8");
    if (!(std::isfinite(f->size_m[i]) && f->size_m[i] > 0.0f)) return refuse(why, "size_m must be finite and positive");
  }
  if (f->z0 < 0 || f->nz <= 0 || (int64_t)f->z0 + f->nz > f->dims[2]) return refuse(why, "stored planes outside the volume");
  // hsk_create's own limit: fewer than 2^32 voxels (64 <= vol_x vol_y, so vol_z, nz < 2^26 and no product below can wrap)
  if ((uint64_t)f->dims[0] * (uint64_t)f->dims[1] >= ((uint64_t)1 << 32) ||
      (uint64_t)f->dims[0] * (uint64_t)f->dims[1] * (uint64_t)f->dims[2] >= ((uint64_t)1 << 32))
    return refuse(why, "dims describe 2^32 voxels or more");
  if (!(std::isfinite(f->trunc_eff_m) && f->trunc_eff_m > 0.0f)) return refuse(why, "the truncation distance must be finite and positive");
  for (size_t i = 156; i < 160; ++i)
    if (p[i] != 0) return refuse(why, "header padding is not zero");
  hsk_volume_info want = *f;
  hskv_finish_info(&want);
  if (f->n_bricks != want.n_bricks) return refuse(why, "brick count does not follow from dims and planes");
  uint64_t sum = 0;
  for (int i = 0; i < 4; ++i) {
    if (f->tsdf_bricks[i] > f->n_bricks) return refuse(why, "a class count exceeds the brick count");
    sum += f->tsdf_bricks[i];
  }
  if (sum != f->n_bricks) return refuse(why, "the class counts do not add up to the brick count");
  if ((f->flags & 1u) ? (f->color_bricks[0] > f->n_bricks || f->color_bricks[1] > f->n_bricks || f->color_bricks[0] + f->color_bricks[1] != f->n_bricks)
                      : (f->color_bricks[0] != 0 || f->color_bricks[1] != 0))
    return refuse(why, "the colour class counts do not add up to the brick count");
  if (f->tsdf_table_bytes != want.tsdf_table_bytes || f->tsdf_payload_bytes != want.tsdf_payload_bytes ||
      f->color_table_bytes != want.color_table_bytes || f->color_payload_bytes != want.color_payload_bytes)
    return refuse(why, "a section length does not follow from the brick counts");
  if (f->total_bytes != want.total_bytes) return refuse(why, "the total length is not the sum of the sections");
  return HSK_OK;
}

int hskv_validate(const void* buf, size_t n_bytes, hsk_volume_info* info, std::string* why) {
  hsk_volume_info f;
  int r = hskv_parse_header(buf, n_bytes, &f, why);
  if (r != HSK_OK) return r;
  if (f.total_bytes != (uint64_t)n_bytes) return refuse(why, n_bytes < f.total_bytes ? "truncated (shorter than its total length)" : "longer than its total length");
  const unsigned char* p = (const unsigned char*)buf;
  r = check_table(p + HSKV_HEADER_BYTES, f.n_bricks, f.tsdf_table_bytes, false, f.tsdf_bricks, why);
  if (r != HSK_OK) return r;
  if (f.flags & 1u) {
    r = check_table(p + HSKV_HEADER_BYTES + f.tsdf_table_bytes + f.tsdf_payload_bytes, f.n_bricks, f.color_table_bytes, true, f.color_bricks, why);
    if (r != HSK_OK) return r;
  }
  *info = f;
  return HSK_OK;
}

int hskv_validate_file(const char* path, hsk_volume_info* info, std::string* why) {
  FILE* fp = fopen(path, "rb");
  if (!fp) return refuse(why, "cannot open the file");
  struct Closer {
    FILE* f;
    ~Closer() { fclose(f); }
  } closer{fp};
  unsigned char head[HSKV_HEADER_BYTES];
  const size_t got = fread(head, 1, sizeof(head), fp);
  hsk_volume_info f;
  int r = hskv_parse_header(head, got, &f, why);
  if (r != HSK_OK) return r;
  if (fseek(fp, 0, SEEK_END) != 0) return refuse(why, "cannot seek in the file");
  const long long len = ftello(fp);
  if (len < 0) return refuse(why, "cannot tell the file's length");
  if ((uint64_t)len != f.total_bytes)
    return refuse(why, (uint64_t)len < f.total_bytes ? "truncated (shorter than its total length)" : "longer than its total length");
  std::vector<unsigned char> tab;
  try {
    tab.resize((size_t)f.tsdf_table_bytes);
  } catch (const std::bad_alloc&) {
    return refuse(why, "out of host memory for the class table");
  }
  if (fseeko(fp, HSKV_HEADER_BYTES, SEEK_SET) != 0 || fread(tab.data(), 1, tab.size(), fp) != tab.size()) return refuse(why, "cannot read the class table");
  r = check_table(tab.data(), f.n_bricks, f.tsdf_table_bytes, false, f.tsdf_bricks, why);
  if (r != HSK_OK) return r;
  if (f.flags & 1u) {
    if (fseeko(fp, (off_t)(HSKV_HEADER_BYTES + f.tsdf_table_bytes + f.tsdf_payload_bytes), SEEK_SET) != 0 ||
        fread(tab.data(), 1, tab.size(), fp) != tab.size())
      return refuse(why, "cannot read the colour class table");
    r = check_table(tab.data(), f.n_bricks, f.color_table_bytes, true, f.color_bricks, why);
    if (r != HSK_OK) return r;
  }
  *info = f;
  return HSK_OK;
}
