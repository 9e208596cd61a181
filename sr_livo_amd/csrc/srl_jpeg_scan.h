// srl_jpeg_scan.h -- the host side of srl_jpeg_decode: the marker walk up to SOS (srl_jpeg_parse) and the baseline Huffman decode of the one
// interleaved scan (srl_jpeg_entropy_decode), both declared in srlivo_hip.h.  Plain C++ without a HIP call and without an allocation, so
// that the file also builds into a stand-alone program under ASan / UBSan (tests/jpeg_scan_san_main.cpp).
#pragma once
#include "../../include/srlivo_hip.h"

#include <cstdint>

// srl_jpeg_entropy_decode, which also reports what the device's 32-bit IDCT is guarded by: the largest sum over one block of
// |coefficient| * table entry (saturated at INT64_MAX / 2).  max_block_l1 may be NULL.
int srl_jpeg_entropy_decode_l1(const uint8_t *bytes, int64_t n, const srl_jpeg_info *info, int16_t *coef, int64_t capacity_blocks, uint16_t qt[3][64],
                               int64_t *max_block_l1);
// the same sum over caller-supplied blocks in natural order with one table (srl_jpeg_idct_blocks)
int64_t srl_jpeg_blocks_l1(const int16_t *coef, int64_t n_blocks, const uint16_t qt[64]);
