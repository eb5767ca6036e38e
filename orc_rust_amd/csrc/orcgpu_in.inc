// orcgpu_in.inc -- the keys of a SQL IN list and the hash set filter_in_kernel probes, host only and free of HIP
// (tests/hostcheck/filter_plan_in_check.cpp compiles this very text under AddressSanitizer + UBSan).  The plan compiler
// (orcgpu_filter_plan.inc) brings every literal to its column's key and collects the keys here; in_build_table lays the table of
// device/filter_program.h into the literal pool.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "device/filter_program.h"

namespace orcgpu_host {

// The usable keys of one IN leaf: literals that can equal a row, brought to the column's key.  One of the three vectors is used.
struct InKeys {
  uint32_t kind = IN_KEY_I64;
  std::vector<uint64_t> k64;                          // integers, Timestamps (as int64), floats (in_float_key)
  std::vector<std::pair<uint64_t, uint64_t>> k128;    // Decimal at the column's scale: {high ^ sign bit, low}, so that pairs sort as int128
  std::vector<std::string> kstr;                      // strings: the bytes
  bool has_null = false;                              // a NULL literal stands in the list

  void add_dec128(uint64_t lo, int64_t hi) { k128.emplace_back((uint64_t)hi ^ (1ull << 63), lo); }
  static int64_t dec_high(const std::pair<uint64_t, uint64_t>& k) { return (int64_t)(k.first ^ (1ull << 63)); }
  // sorted, each key once
  void dedup() {
    std::sort(k64.begin(), k64.end());
    k64.erase(std::unique(k64.begin(), k64.end()), k64.end());
    std::sort(k128.begin(), k128.end());
    k128.erase(std::unique(k128.begin(), k128.end()), k128.end());
    std::sort(kstr.begin(), kstr.end());
    kstr.erase(std::unique(kstr.begin(), kstr.end()), kstr.end());
  }
  size_t size() const { return kind == IN_KEY_I64 ? k64.size() : kind == IN_KEY_DEC128 ? k128.size() : kstr.size(); }
};

// little-endian words into the literal pool (the IN tables here, the LIKE patterns of orcgpu_filter_plan.inc)
inline void put32(std::vector<uint8_t>& pool, size_t at, uint32_t v) {
  for (int b = 0; b < 4; b++) pool[at + b] = (uint8_t)(v >> (8 * b));
}
inline void put64(std::vector<uint8_t>& pool, size_t at, uint64_t v) {
  for (int b = 0; b < 8; b++) pool[at + b] = (uint8_t)(v >> (8 * b));
}

// The hash set of `keys` (deduplicated, at least one) appended to the pool, 8-byte aligned: where it starts; `len` gets its bytes.
inline uint64_t in_build_table(const InKeys& keys, uint32_t flags, std::vector<uint8_t>& pool, uint32_t& len) {
  while (pool.size() & 7) pool.push_back(0);
  const uint64_t base = pool.size();
  const uint32_t n = (uint32_t)keys.size();
  uint32_t n_slots = 4;
  while (n_slots < 2 * n) n_slots <<= 1;
  const uint32_t slot_bytes = keys.kind == IN_KEY_I64 ? 8 : 16, occ_words = (n_slots + 63) / 64;
  const size_t o_occ = kInHeaderBytes, o_slots = o_occ + (size_t)occ_words * 8, o_bytes = o_slots + (size_t)n_slots * slot_bytes;
  size_t total = o_bytes;
  uint32_t min_len = 0, max_len = 0;
  if (keys.kind == IN_KEY_STRING) {
    min_len = 0xffffffffu;
    for (const std::string& s : keys.kstr) {
      total += s.size();
      min_len = std::min<uint32_t>(min_len, (uint32_t)s.size());
      max_len = std::max<uint32_t>(max_len, (uint32_t)s.size());
    }
  }
  total = (total + 7) & ~(size_t)7;
  pool.resize(base + total, 0);
  const uint32_t header[8] = {keys.kind, n_slots, n, min_len, max_len, flags, 0, 0};
  for (int w = 0; w < 8; w++) put32(pool, base + 4 * w, header[w]);
  std::vector<uint64_t> occ(occ_words, 0);
  auto claim = [&](uint32_t hash) {  // the first free slot at or behind the hash's own
    uint32_t s = hash & (n_slots - 1);
    while ((occ[s >> 6] >> (s & 63)) & 1) s = (s + 1) & (n_slots - 1);
    occ[s >> 6] |= 1ull << (s & 63);
    return s;
  };
  if (keys.kind == IN_KEY_I64) {
    for (uint64_t k : keys.k64) put64(pool, base + o_slots + 8 * (size_t)claim(in_hash_i64(k)), k);
  } else if (keys.kind == IN_KEY_DEC128) {
    for (auto& k : keys.k128) {
      const uint64_t hi = (uint64_t)InKeys::dec_high(k), lo = k.second;
      const size_t at = base + o_slots + 16 * (size_t)claim(in_hash_dec128(lo, hi));
      put64(pool, at, lo);
      put64(pool, at + 8, hi);
    }
  } else {
    size_t off = o_bytes;
    for (const std::string& s : keys.kstr) {
      const uint32_t h = in_hash_bytes(reinterpret_cast<const uint8_t*>(s.data()), (uint32_t)s.size());
      const size_t at = base + o_slots + 16 * (size_t)claim(h);
      put32(pool, at, h);
      put32(pool, at + 4, (uint32_t)s.size());
      put32(pool, at + 8, (uint32_t)off);
      if (!s.empty()) memcpy(pool.data() + base + off, s.data(), s.size());
      off += s.size();
    }
  }
  for (uint32_t w = 0; w < occ_words; w++) put64(pool, base + o_occ + 8 * (size_t)w, occ[w]);
  len = (uint32_t)total;
  return base;
}

}  // namespace orcgpu_host
