// key_map_program.h -- what the host and the kernels of a key map share (include/orcgpu.h: "Key maps and lookup columns"): the kinds
// a stored value has, where a key's values lie, and the probe that FINDS a key's slot in a sealed table of filter_program.h.
// Plain C++: no HIP in here -- tests/hostcheck/key_map_check.cpp compiles it for the host.
#pragma once
#include <stdint.h>

#include "filter_program.h"

// A stored value: 8 bytes (an int64; the bits of a double) or 16 (a Decimal128, little-endian halves).  The numbers are CK_* of
// compute_kernels.hip: a lookup column is laid out as a computed column of the same kind is.
enum { KMV_INT64 = 0, KMV_DEC128 = 1, KMV_F64 = 2 };
constexpr uint32_t kKeyMapMaxValues = 8;         // = ORCGPU_KEY_MAP_MAX_VALUES
constexpr uint32_t kKeyMapNoSlot = 0xffffffffu;  // in_find_i64: the key is not in the table
constexpr unsigned long long kKeyMapSentinel = 0x8080808080808080ull;  // = kKeySetSentinel: a free slot while the table is built

FILTER_HD inline uint32_t key_map_value_width(uint32_t kind) { return kind == KMV_DEC128 ? 16u : 8u; }

// in_probe_i64 that says WHERE: the slot that holds `key`, or kKeyMapNoSlot.  At most n_slots steps, ended by the key or by a free
// slot; the slot index is masked at every step.
FILTER_HD inline uint32_t in_find_i64(const InTable& t, unsigned long long key) {
  const uint32_t mask = t.n_slots - 1;
  uint32_t s = in_first_slot(in_hash_i64(key), t.hash_mask, mask);
  for (uint32_t step = 0; step < t.n_slots; step++, s = (s + 1) & mask) {
    if (!((t.occ[s >> 6] >> (s & 63)) & 1)) return kKeyMapNoSlot;
    if (reinterpret_cast<const unsigned long long*>(t.slots)[s] == key) return s;
  }
  return kKeyMapNoSlot;
}

// Where the values of the key in slot `slot` lie in a value plane of n_slots + 1 entries: at the slot's index -- but for the key
// whose value is the sentinel's, which took no slot while the map was built (its values were written before it had one): entry
// n_slots.  slot < n_slots.
FILTER_HD inline uint32_t key_map_value_index(uint32_t slot, unsigned long long key, uint32_t n_slots) { return key == kKeyMapSentinel ? n_slots : slot; }
