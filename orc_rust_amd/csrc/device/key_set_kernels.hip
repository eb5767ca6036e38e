// key_set_kernels.hip -- the BUILD side of a semi-join: the distinct non-NULL keys of one integer column over the kept rows of
// decoded stripes, collected into a device-resident hash set (include/orcgpu.h: orcgpu_key_set) which the row filter's IN
// machinery then probes (filter_kernels.hip: filter_in_kernel, through a FOP_IN_SET leaf).  The reference has no such thing.
//
// The set's one allocation is the sealed table of filter_program.h from its first byte on -- header (32 bytes), occupancy bitmap,
// n_slots x uint64 slots -- so that sealing moves nothing:
//
//   key_set_insert_kernel   per collected stripe, behind the row filter's evaluation on its stream.  One lane per input row, a
//                           wavefront trip per 64-bit word of the keep mask (filter_words / filter_row / filter_valid /
//                           filter_load_i64: the row access of filter_access.h).  A kept, valid row's key goes into the slots by
//                           linear probing from in_first_slot(in_hash_i64(key), hash_mask, n_slots - 1) -- the hash and the
//                           first slot filter_in_kernel probes with.  A slot has no spare "empty" value (every int64 is a legal key), so the build runs against a
//                           SENTINEL, kKeySetSentinel: a free slot holds it, a lane claims one with a 64-bit compare-and-swap, and a
//                           key EQUAL to the sentinel takes no slot but sets KEY_SET_HAS_SENTINEL.  New keys are counted by ballot
//                           and popcount, one integer add per block; a kept NULL row sets KEY_SET_HAS_NULL.  A probe ends after at
//                           most n_slots steps.  Once the count passes max_keys KEY_SET_OVERFLOW is set, sticky: lanes stop
//                           inserting, later launches leave at once.
//   key_set_seal_kernel     phase 0: the header, and the occupancy bitmap from "slot != sentinel", a ballot per word.  Phase 1, a
//                           launch of one wavefront behind it: the sentinel-valued key, if flagged, becomes an ordinary occupied
//                           slot -- the first free slot of its probe chain already HOLDS its value, so the occupancy bit is all
//                           that is set.  in_table() and in_probe_i64() then work on the table as on any IN list's.
//
// THE CONTRACT.  Integer atomics decide slots, flags and counts: which lane wins a slot, and so where a key lies, may differ from
// run to run.  The set's membership, n_keys and has_null may not: a key is counted by exactly the one lane whose compare-and-swap
// (or, for the sentinel's value, whose atomic OR) changed memory, and a slot never changes again once it holds a key -- so a stale
// load can only show a slot free that is taken, which the compare-and-swap then answers.  No floating point anywhere.
// Bounds: nothing read back from memory is used as an index unmasked -- a slot index is (hash + step) & (n_slots - 1), n_slots is
// the host's; a row is addressed through filter_row, whose loads stay in bounds for rows past n_in.  ORCGPU_POISON covers the
// whole table before the slots are set to the sentinel (orcgpu_key_set_create), so nothing depends on what the memory held.
// How long a launch can run: the table holds at least 2 x max_keys slots and a block adds its new keys when it ends, after at most
// a few trips per wavefront; a lane that finds the table FULL (n_slots steps, no free slot, no match) sets KEY_SET_OVERFLOW itself,
// and every probe looks at the flag again each 1024 steps.
//
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): in front of each kernel.  No kernel uses scratch.
#pragma once
#include <stdint.h>

#include "filter_program.h"
#include "filter_access.h"
#include "agg_kernels.hip"

// A free slot while the set is built.  Its bytes are all 0x80, so one hipMemsetAsync lays it over the slots.
constexpr unsigned long long kKeySetSentinel = 0x8080808080808080ull;
enum { KEY_SET_OVERFLOW = 1, KEY_SET_HAS_NULL = 2, KEY_SET_HAS_SENTINEL = 4 };
// The set's control words, behind the table in its allocation; zeroed when the set is created, fetched by the seal's one wait
struct KeySetControl {
  uint32_t n_keys;  // distinct non-NULL keys so far, the sentinel's value included (above max_keys: KEY_SET_OVERFLOW is set)
  uint32_t flags;   // KEY_SET_*
};

// Resource usage (gfx950): 24 VGPRs, 103 SGPRs, no scratch, no spill, 16 bytes of LDS; occupancy 7 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
key_set_insert_kernel(KeptRows rows, uint32_t col, unsigned long long* slots, uint32_t n_slots, uint32_t max_keys, uint32_t hash_mask, KeySetControl* ctl) {
  __shared__ uint32_t new_s[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, mask = n_slots - 1;
  const FilterCol c = rows.cols[col];
  const FilterWords ws = filter_words(rows.n_in);
  uint32_t n_new = 0;  // (wave-uniform: popcounts of ballots)
  bool has_null = false, full = false;
  for (uint64_t w = ws.first; w < ws.n; w += ws.stride) {
    if (__atomic_load_n(&ctl->flags, __ATOMIC_RELAXED) & KEY_SET_OVERFLOW) break;  // (the set is refused: nothing more goes in)
    const unsigned long long m = agg_keep_word(rows, w);
    if (!m) continue;
    const uint64_t j = w * 64 + lane;
    const FilterRow r = filter_row(rows, j);
    const bool kept = ((m >> lane) & 1) && r.live;
    const bool valid = kept && filter_valid(c, r.u, r.l, rows.W);
    has_null = has_null || (kept && !valid);
    bool is_new = false;
    if (valid) {
      const unsigned long long key = (unsigned long long)filter_load_i64(c, r.row);
      if (key == kKeySetSentinel) {
        if (!(__atomic_load_n(&ctl->flags, __ATOMIC_RELAXED) & KEY_SET_HAS_SENTINEL))
          is_new = !(atomicOr(&ctl->flags, (uint32_t)KEY_SET_HAS_SENTINEL) & KEY_SET_HAS_SENTINEL);
      } else {
        bool done = false;
        uint32_t s = in_first_slot(in_hash_i64(key), hash_mask, mask);
        for (uint32_t step = 0; step < n_slots && !done; step++, s = (s + 1) & mask) {
          if ((step & 1023) == 1023 && (__atomic_load_n(&ctl->flags, __ATOMIC_RELAXED) & KEY_SET_OVERFLOW)) {
            done = true;  // (refused meanwhile: the key is dropped with the set)
            break;
          }
          unsigned long long cur = __atomic_load_n(&slots[s], __ATOMIC_RELAXED);
          if (cur == kKeySetSentinel) {
            cur = atomicCAS(&slots[s], kKeySetSentinel, key);
            if (cur == kKeySetSentinel) {
              is_new = true;
              done = true;
            }
          }
          if (cur == key) done = true;
        }
        full = full || !done;  // (n_slots steps, neither the key nor a free slot: more than max_keys keys are in)
      }
    }
    n_new += (uint32_t)__builtin_popcountll(__ballot(is_new));
  }
  if (__ballot(full) && lane == 0) atomicOr(&ctl->flags, (uint32_t)KEY_SET_OVERFLOW);
  if (__ballot(has_null) && lane == 0 && !(__atomic_load_n(&ctl->flags, __ATOMIC_RELAXED) & KEY_SET_HAS_NULL)) atomicOr(&ctl->flags, (uint32_t)KEY_SET_HAS_NULL);
  if (lane == 0) new_s[wave] = n_new;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t n = new_s[0] + new_s[1] + new_s[2] + new_s[3];
    if (n && atomicAdd(&ctl->n_keys, n) + n > max_keys) atomicOr(&ctl->flags, (uint32_t)KEY_SET_OVERFLOW);
  }
}

// tab: the set's table (header, occupancy, slots), n_slots a power of two >= 64.  phase 0, any grid of 256-thread blocks: the header
// and the occupancy words; phase 1, <<<1, 64>>> behind it: the sentinel's value as a key.  An overflowed set is left as it is: the
// host refuses it behind the wait.
// Resource usage (gfx950): 9 VGPRs, 33 SGPRs, no scratch, no spill, no LDS; occupancy 8 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
key_set_seal_kernel(uint8_t* tab, uint32_t n_slots, uint32_t hash_mask, const KeySetControl* ctl, uint32_t phase) {
  const uint32_t lane = threadIdx.x & 63, mask = n_slots - 1;
  const uint32_t occ_words = n_slots / 64;
  unsigned long long* occ = reinterpret_cast<unsigned long long*>(tab + kInHeaderBytes);
  const unsigned long long* slots = occ + occ_words;
  const uint32_t flags = ctl->flags;
  if (flags & KEY_SET_OVERFLOW) return;
  if (phase == 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      uint32_t* h = reinterpret_cast<uint32_t*>(tab);
      h[0] = IN_KEY_I64;
      h[1] = n_slots;
      h[2] = ctl->n_keys;
      h[3] = h[4] = 0;
      h[5] = flags & KEY_SET_HAS_NULL ? (uint32_t)IN_HAS_NULL : 0u;
      h[6] = ~hash_mask;
      h[7] = 0;
    }
    const uint64_t first = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), stride = (uint64_t)gridDim.x * 4;
    for (uint64_t w = first; w < occ_words; w += stride) {
      const unsigned long long M = __ballot(slots[w * 64 + lane] != kKeySetSentinel);
      if (lane == 0) occ[w] = M;
    }
    return;
  }
  if (!(flags & KEY_SET_HAS_SENTINEL) || blockIdx.x || threadIdx.x) return;
  // the first free slot of the sentinel's chain: it holds the sentinel, which is the key's own value
  uint32_t s = in_first_slot(in_hash_i64(kKeySetSentinel), hash_mask, mask);
  for (uint32_t step = 0; step < n_slots; step++, s = (s + 1) & mask) {
    if (slots[s] != kKeySetSentinel) continue;
    occ[s >> 6] |= 1ull << (s & 63);
    return;
  }
}
