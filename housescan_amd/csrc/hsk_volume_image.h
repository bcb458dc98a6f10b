// hsk_volume_image.h -- the "HSKV" version 1 sparse volume image on the host side: the header's byte offsets,
// its writer and the validator hsk_volume_image_info / hsk_unpack_volume share.  Little-endian; host only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/hskinfu.h"

#define HSKV_HEADER_BYTES 256
#define HSKV_VERSION 1
// byte offsets of the header's fields
#define HSKV_AT_MAGIC 0            // "HSKV"
#define HSKV_AT_VERSION 4          // u32
#define HSKV_AT_HEADER_BYTES 8     // u32 = 256
#define HSKV_AT_FLAGS 12           // u32, bit 0: colour present
#define HSKV_AT_DIMS 16            // i32[3]
#define HSKV_AT_Z0 28              // i32
#define HSKV_AT_NZ 32              // i32
#define HSKV_AT_SIZE_M 36          // f32[3]
#define HSKV_AT_TRUNC 48           // f32 configured trunc_dist_m
#define HSKV_AT_TRUNC_EFF 52       // f32 effective (VolParams::tau)
#define HSKV_AT_WIDTH 56           // i32
#define HSKV_AT_HEIGHT 60          // i32
#define HSKV_AT_INTR 64            // f32 fx fy cx cy
#define HSKV_AT_POSE 80            // f32[16]
#define HSKV_AT_FRAME 144          // i32
#define HSKV_AT_COLOR_MAXW 148     // i32
#define HSKV_AT_COLOR_BAND 152     // f32
                                   // 156: u32 0
#define HSKV_AT_N_BRICKS 160       // u64
#define HSKV_AT_TSDF_BRICKS 168    // u64[4] by class
#define HSKV_AT_COLOR_BRICKS 200   // u64[2]: ZERO, RAW
#define HSKV_AT_TSDF_TABLE 216     // u64 bytes
#define HSKV_AT_TSDF_PAYLOAD 224   // u64 bytes
#define HSKV_AT_COLOR_TABLE 232    // u64 bytes
#define HSKV_AT_COLOR_PAYLOAD 240  // u64 bytes
#define HSKV_AT_TOTAL 248          // u64 bytes

#define HSKV_REC_UNIFORM 4
#define HSKV_REC_SPLIT 516
#define HSKV_REC_RAW 2048

// bricks of a volume of these stored planes, and the bytes of a class table of so many bricks
uint64_t hskv_bricks(const int32_t dims[3], int32_t nz);
uint64_t hskv_table_bytes(uint64_t n_bricks);
// fills the section lengths and the total of *info from its dims, nz, flags and brick counts
void hskv_finish_info(hsk_volume_info* info);
void hskv_write_header(const hsk_volume_info* info, unsigned char out[HSKV_HEADER_BYTES]);
// the header alone (n_bytes >= 256): magic, version, header size, self-consistency.  HSK_OK or HSK_ERR_ARG with *why
int hskv_parse_header(const void* buf, size_t n_bytes, hsk_volume_info* info, std::string* why);
// the whole image: the header, total == n_bytes, every class byte legal, the header's counts and lengths those of the tables
int hskv_validate(const void* buf, size_t n_bytes, hsk_volume_info* info, std::string* why);
// the same for a file: reads the header and the class tables only
int hskv_validate_file(const char* path, hsk_volume_info* info, std::string* why);
