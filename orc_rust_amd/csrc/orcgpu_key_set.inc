// orcgpu_key_set.inc -- what a device-resident key set (include/orcgpu.h: orcgpu_key_set) works out on the host with plain
// arithmetic: how many slots a limit takes and where the table's parts lie (key_set_layout), the hash mask of
// ORCGPU_KEY_SET_HASH_BITS (key_set_hash_mask), which columns may be a key (key_set_column_check), what the plan compiler is told
// of a set a predicate names (KeySetRef), and the sealed table as the host would build it (key_set_build_host: what
// key_set_seal_kernel leaves, up to where a key lies in its chain).  No HIP in this file and nothing of the context:
// tests/hostcheck/key_set_check.cpp compiles it for the host, under AddressSanitizer + UBSan.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "device/filter_program.h"

namespace orcgpu_host {

static_assert(ORCGPU_KEY_SET_MAX_KEYS == (1u << 26) && ORCGPU_PRED_IN_SET == 26, "the key set of include/orcgpu.h");

constexpr unsigned long long kKeySetFree = 0x8080808080808080ull;  // kKeySetSentinel (device/key_set_kernels.hip): a free slot while the set is built
constexpr uint32_t kKeySetMinSlots = 64;                           // (whole occupancy words)

// One allocation: the sealed table of filter_program.h -- header, occupancy, slots -- and behind it the control words
struct KeySetLayout {
  uint32_t n_slots = 0;
  uint64_t o_occ = 0, o_slots = 0, table_bytes = 0, o_ctl = 0, bytes = 0;
};
// false: max_keys is not 1 .. ORCGPU_KEY_SET_MAX_KEYS.  Slots: the power of two >= 2 x max_keys, at least 64 -- at most 2^27, so
// that the table's bytes (1 GiB of slots, 16 MiB of occupancy, the header) stay inside the 32 bits FilterInsn::lit_len carries.
inline bool key_set_layout(uint64_t max_keys, KeySetLayout& out) {
  out = KeySetLayout{};
  if (!max_keys || max_keys > ORCGPU_KEY_SET_MAX_KEYS) return false;
  uint64_t n = kKeySetMinSlots;
  while (n < 2 * max_keys) n <<= 1;
  out.n_slots = (uint32_t)n;
  out.o_occ = kInHeaderBytes;
  out.o_slots = out.o_occ + n / 64 * 8;
  out.table_bytes = out.o_slots + n * 8;
  out.o_ctl = (out.table_bytes + 255) / 256 * 256;
  out.bytes = out.o_ctl + 256;
  return out.table_bytes <= 0xffffffffull;
}

// ORCGPU_KEY_SET_HASH_BITS = N (1 .. 32): the build and the probe of a set use the low N bits of a key's hash -- long probe
// chains that start in the table's last slots and wrap round its end (in_first_slot), the same membership.  Anything else: all
// 32 bits.  Read when a set is created; the mask is the set's from then on and travels in its table's header, so that no probe can
// disagree with the build.
inline uint32_t key_set_hash_mask(const char* env) {
  if (!env || !*env) return 0xffffffffu;
  const long n = strtol(env, nullptr, 10);
  return n >= 1 && n < 32 ? (uint32_t)((1ull << n) - 1) : 0xffffffffu;
}

// May a column of this ORC type be a key -- of the build side or of the probe side?  Byte, Short, Int, Long and Date are, all as
// int64.  ORCGPU_UNSUPPORTED with the column's name in `err` otherwise.  (`what`: "key set" or "row filter", who refuses.)
inline int key_set_column_check(int32_t orc_type, bool dict_read, bool nested, const char* name, const char* what, char* err, size_t n) {
  const char* why = nullptr;
  switch (orc_type) {
    case ORCGPU_T_BYTE: case ORCGPU_T_SHORT: case ORCGPU_T_INT: case ORCGPU_T_LONG: case ORCGPU_T_DATE: break;
    case ORCGPU_T_TIMESTAMP: case ORCGPU_T_TIMESTAMP_INSTANT: why = "a Timestamp column (the units and zones of two files need not agree)"; break;
    case ORCGPU_T_DECIMAL: why = "a Decimal column"; break;
    case ORCGPU_T_FLOAT: case ORCGPU_T_DOUBLE: why = "a Float / Double column"; break;
    case ORCGPU_T_BOOLEAN: why = "a Boolean column"; break;
    case ORCGPU_T_STRING: case ORCGPU_T_VARCHAR: case ORCGPU_T_CHAR: case ORCGPU_T_BINARY: why = "a String / Varchar / Char / Binary column"; break;
    default: why = "a nested column or one of an unknown kind"; break;
  }
  if (!why && nested) why = "a nested column";
  if (!why && dict_read) why = "read as a dictionary column";
  if (!why) return ORCGPU_OK;
  snprintf(err, n, "%s: column '%s' is %s: the keys of a key set are Byte, Short, Int, Long and Date columns", what, name ? name : "", why);
  return ORCGPU_UNSUPPORTED;
}

// What the plan compiler learns of a set of its context when a predicate names it (ORCGPU_PRED_IN_SET)
enum { KEY_SET_BUILDING = 0, KEY_SET_SEALED = 1, KEY_SET_FAILED = 2 };
struct KeySetRef {
  uint64_t id = 0;
  int state = KEY_SET_BUILDING;
  uint64_t table = 0;   // the sealed table's device address ...
  uint32_t bytes = 0;   // ... and its bytes
  uint32_t n_keys = 0;
  uint32_t max_keys = 0;
  bool has_null = false;
  std::shared_ptr<void> hold;  // the set's memory: a plan that names the table keeps it alive
};
typedef std::vector<KeySetRef> KeySetRefs;

// The sealed table of `keys` (distinct, at most max_keys) as key_set_seal_kernel leaves it, on the host.  Which of two colliding
// keys lies first in a chain is the insertion order's here and a race's on the device; what a probe answers is the same.
inline bool key_set_build_host(const uint64_t* keys, size_t n, bool has_null, uint64_t max_keys, uint32_t hash_mask, std::vector<uint8_t>& tab) {
  KeySetLayout lay;
  if (!key_set_layout(max_keys, lay) || n > max_keys) return false;
  tab.assign(lay.table_bytes, 0);
  uint32_t* h = reinterpret_cast<uint32_t*>(tab.data());
  uint64_t* occ = reinterpret_cast<uint64_t*>(tab.data() + lay.o_occ);
  uint64_t* slots = reinterpret_cast<uint64_t*>(tab.data() + lay.o_slots);
  const uint32_t mask = lay.n_slots - 1;
  for (uint32_t s = 0; s < lay.n_slots; s++) slots[s] = kKeySetFree;
  for (size_t k = 0; k < n; k++) {
    uint32_t s = in_first_slot(in_hash_i64(keys[k]), hash_mask, mask);
    while ((occ[s >> 6] >> (s & 63)) & 1) s = (s + 1) & mask;
    occ[s >> 6] |= 1ull << (s & 63);
    slots[s] = keys[k];
  }
  h[0] = IN_KEY_I64;
  h[1] = lay.n_slots;
  h[2] = (uint32_t)n;
  h[5] = has_null ? (uint32_t)IN_HAS_NULL : 0u;
  h[6] = ~hash_mask;
  return true;
}

}  // namespace orcgpu_host
