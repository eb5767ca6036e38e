// top_k_program.h -- what the host and the kernels of ORDER BY ... LIMIT k share (device/top_k_kernels.hip, orcgpu_top_k_host.inc):
// the sort keys as a kernel argument, the state of the radix select, and the KEY STRING -- the bytes whose plain unsigned order is
// the order of include/orcgpu.h ("Top-k").  No HIP in this file: tests/hostcheck/top_k_host_check.cpp compiles it for the host.
//
// The key string of a row: per key, most significant key first, ONE NULL BYTE and then 8 value bytes (16 for a Decimal key), most
// significant byte first.
//   null byte     nulls_first: NULL 0, a value 1; else: a value 0, NULL 1.  `descending` does not touch it.
//   value bytes   the value's unsigned IMAGE, every byte inverted under `descending`; all 0 for a NULL (the null byte has decided).
//   images        integers, Date, Timestamp units: the int64 with its sign bit flipped.  Boolean: 0 or 1.  Decimal: the unscaled
//                 128-bit value with its sign bit flipped.  Float / Double: the double (a Float widened) -- every NaN ~0, -0.0 taken
//                 as +0.0, then a negative's bits inverted and a non-negative's sign bit set: -inf < finite < +inf < NaN.
// Rows with equal key strings are equal in every key.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define TOPK_HD __host__ __device__ __forceinline__
#else
#define TOPK_HD inline
#endif

constexpr uint32_t kTopKMaxKeys = 4;       // ORCGPU_TOP_K_MAX_KEYS
constexpr uint32_t kTopKMax = 65536;       // ORCGPU_TOP_K_MAX
constexpr uint32_t kTopKMaxLen = kTopKMaxKeys * 17;  // bytes of the longest key string: four Decimal keys
constexpr uint32_t kTopKEveryBin = 256;    // TopKState::bin: "every candidate is a winner" (fewer candidates than asked for)
constexpr uint32_t kTopKSortTile = 2048;   // winners a block of the sort takes: 8 words for each of its 4 wavefronts

enum { TK_INT = 0, TK_BOOL = 1, TK_FLOAT = 2, TK_DEC128 = 3 };

struct TopKKey {
  uint32_t col;          // column of the result
  uint32_t kind;         // TK_*
  uint32_t descending, nulls_first;
  uint32_t first;        // where its null byte stands in the key string
  uint32_t bytes;        // 9 or 17: the null byte and the value bytes
};
struct TopKKeys {        // a kernel argument, by value
  uint32_t n, len;       // keys; bytes of the key string = passes of the select = passes of the sort
  TopKKey key[kTopKMaxKeys];
};

// The radix select's state on the device, zeroed in front of every call.  top_k_choose_kernel writes it, one pass after the other.
struct TopKState {
  uint32_t remaining;    // rows still to take from the candidates
  uint32_t done;         // nothing is left to decide: the candidates are exactly the remainder, or fewer
  uint32_t last;         // the last pass that chose a bin
  uint32_t kept;         // candidates in front of pass 0: the rows the predicate kept
  uint32_t bin[kTopKMaxLen + 4];  // per pass the chosen byte (kTopKEveryBin: every candidate wins)
};

TOPK_HD uint64_t top_k_image_i64(int64_t v) { return (uint64_t)v ^ (1ull << 63); }
TOPK_HD uint64_t top_k_image_f64(double d) {
  if (d != d) return ~0ull;  // every NaN, above +inf (whose image is 0xfff0...0)
  if (d == 0.0) d = 0.0;     // -0.0 = 0.0
  uint64_t b;
  memcpy(&b, &d, 8);
  return (b >> 63) ? ~b : b | (1ull << 63);
}
TOPK_HD uint64_t top_k_image_dec_hi(uint64_t hi) { return hi ^ (1ull << 63); }
// value byte b (0: the most significant) of an image of `n` = 8 bytes (lo) or 16 (hi, lo)
TOPK_HD uint32_t top_k_image_byte(uint64_t hi, uint64_t lo, uint32_t n, uint32_t b) {
  if (n == 16 && b < 8) return (uint32_t)(hi >> (8 * (7 - b))) & 255u;
  return (uint32_t)(lo >> (8 * ((n - 1 - b) & 7))) & 255u;
}
// byte b of a key's part of the string (0: the null byte) from what a row holds for it
TOPK_HD uint32_t top_k_key_byte(const TopKKey& k, bool valid, uint64_t hi, uint64_t lo, uint32_t b) {
  if (b == 0) return (valid ? 1u : 0u) ^ (k.nulls_first ? 0u : 1u);
  if (!valid) return 0;
  const uint32_t v = top_k_image_byte(hi, lo, k.bytes - 1, b - 1);
  return k.descending ? v ^ 255u : v;
}
