// agg_group_program.h -- GROUP BY for the aggregates: the key list as the host compiles it (orcgpu_group_plan.inc) and the kernels of
// agg_group_kernels.hip run it, the limits both sides share, and the record a group's key travels in.  Plain C++: no HIP in here.
#pragma once
#include <stdint.h>

#include "agg_program.h"

constexpr uint32_t kGroupMaxKeys = 4;       // ORCGPU_GROUP_MAX_KEYS
constexpr uint32_t kGroupMax = 256;         // ORCGPU_GROUP_MAX: groups of one result
constexpr uint32_t kGroupKeyBytes = 64;     // ORCGPU_GROUP_KEY_BYTES: a String key value's bytes
constexpr uint32_t kGroupSlots = 1024;      // the open-addressing table group_assign_kernel probes: four slots a group at the limit
constexpr uint32_t kGroupNoSlot = 0xffffffffu;
// The wide path (agg_group_wide_kernels.hip), taken when the limit of groups in one result is set above kGroupMax
constexpr uint32_t kGroupLimitMax = 1u << 20;   // ORCGPU_GROUP_LIMIT_MAX: the highest limit of groups in one result
constexpr uint32_t kGroupWideTile = 2048;       // input rows, and sorted pairs, a block of the wide kernels takes: 4 wavefronts x 8 words
constexpr uint32_t kGroupRadixBits = 8;         // bits of the group number a pass of the sort takes

// The key columns, by value into every kernel.  hash_mask: the bits of a key tuple's hash that are kept (ORCGPU_GROUP_HASH_BITS)
struct GroupKeys {
  uint32_t n;
  uint32_t hash_mask;
  uint32_t col[kGroupMaxKeys];    // index into the FilterCol table
  uint32_t fkind[kGroupMaxKeys];  // FKIND_INT / _BOOL / _DEC128 / _STRING: how a value is loaded and compared
};

// A slot of the table: claim = the input row that claimed it, + 1 (0: free); first_inv = ~(the smallest kept input row with the
// slot's key) as atomicMax leaves it, so that a zeroed table is an empty one
struct GroupSlot {
  unsigned long long claim;
  unsigned long long first_inv;
};

// What the kernels leave for the host beside the records: flags, the groups found, the slots claimed
enum { GROUP_TOO_MANY = 1, GROUP_KEY_TOO_LONG = 2 /* << key: bits 1 .. 4 */ };
struct GroupControl {
  uint32_t flags;     // GROUP_*
  uint32_t n_groups;  // group_number_kernel: occupied slots (may pass kGroupMax: GROUP_TOO_MANY is set then)
  uint32_t claimed;   // group_assign_kernel: slots claimed so far
  uint32_t kept;      // the wide path only: the kept rows, which are the pairs its sort moves (else 0)
};

// The key of a group in one key column, from the group's first row: w = the int64 (sign-extended into w[1]), the Boolean as 0 / 1
// or the Decimal's unscaled 128 bits; strings: len and the bytes (the first kGroupKeyBytes of a longer one, which is refused)
struct GroupKeyRecord {
  uint32_t is_null;
  uint32_t len;
  unsigned long long w[2];
  uint8_t bytes[kGroupKeyBytes];
};

// Blocks of agg_group_partial_kernel's grid along x: a function of the input row count alone, like agg_blocks, but capped lower:
// a block leaves a record per (instruction, group), not one per instruction
constexpr uint32_t kAggGroupMaxBlocks = 128;
inline uint32_t agg_group_blocks(uint64_t n_in) {
  const uint64_t n_words = (n_in + 63) / 64, b = (n_words + 3) / 4;
  return (uint32_t)(b < kAggGroupMaxBlocks ? (b ? b : 1) : kAggGroupMaxBlocks);
}
