// key_map_kernels.hip -- a many-to-one equi-join in two kernels (include/orcgpu.h: "Key maps and lookup columns"): the BUILD side
// keeps chosen columns beside its unique keys in HBM, the PROBE side gets them as ordinary columns.  The reference has no such thing.
//
// A key map is a key set (key_set_kernels.hip) whose allocation carries, behind the table and the control words, per value column
// a VALUE PLANE of n_slots + 1 entries of 8 or 16 bytes and a VALIDITY PLANE of n_slots + 1 bytes, both indexed by the slot a key
// holds; entry n_slots belongs to the key whose value is the sentinel's (it takes no slot while the map is built).
//
//   key_map_insert_kernel   key_set_insert_kernel's walk, probing and counting, against the same slot array.  The lane whose
//                           compare-and-swap CLAIMS slot s writes its row's values into the planes at s, with plain stores: nobody
//                           else writes there (a slot is claimed once), nobody reads before the seal's wait.  A lane that finds its
//                           own key already present -- a slot that holds it, or for the sentinel's value the flag already set --
//                           sets KEY_MAP_DUPLICATE, sticky, and writes nothing.  A NULL value stores 0 and validity byte 0.
//   lookup_columns_kernel   inside the decode call, behind the last kernel that writes a column and in front of
//                           compute_columns_kernel and the summary's copy.  grid (ceil(n_batches * W / 4), pairs) x 256;
//                           blockIdx.y = one (map, probe key column) pair (its LookupJob).  A wavefront takes ONE validity word of
//                           the output with compute_columns_kernel's geometry; a lane loads its row's key through filter_access.h,
//                           probes ONCE (in_find_i64: in_first_slot(in_hash_i64(key), ...), occupancy, slots), and for every value
//                           column of the pair copies the 8- or 16-byte value -- 0 where NULL --; the ballot of "valid" is the
//                           validity word, its popcount goes to the batch's null count.  NULL: the key is NULL, the map has no such
//                           key, the stored value is NULL.  The table (header, occupancy, slots) is staged in LDS when it fits
//                           kInLdsBytes, as filter_in_kernel stages it, else probed in global memory; the planes are always read
//                           from global memory.
//
// What may race.  Insert: integer atomics decide slots, flags and the count -- which of two rows with one key came first may differ
// from run to run; that the duplicate flag is set may not: it is set exactly when some insert found its own key present, and of two
// inserts of one key exactly one claims.  Probe: the null counts, integer adds of popcounts.  No floating-point atomic, no atomic
// that decides a value.
// Bounds.  Insert: a slot index is (hash + step) & (n_slots - 1) with the host's n_slots; a plane index is that slot or n_slots;
// rows through filter_row as in the set's kernel; a value's column index comes from the host's table and is checked below n_cols.
// Probe: the word, batch and row clamps of compute_columns_kernel (a dead lane loads and stores nothing); the table's header is
// checked against its bytes by in_table and its n_slots against the host's, so a plane index is a masked slot < n_slots or n_slots
// itself; n_values is clamped to 8.  Chains end after n_slots steps; the insert re-reads the overflow flag every 1024 steps.
// Plain C++: no inline assembly.
//
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): in front of each kernel.
#pragma once
#include <stdint.h>

#include "filter_access.h"
#include "key_map_program.h"
#include "key_set_kernels.hip"

enum { KEY_MAP_DUPLICATE = 8 };  // beside KEY_SET_* in KeySetControl::flags

// One value column of an insert: where it is read and where it goes
struct KeyMapValueJob {
  uint32_t col;    // the result's column
  uint32_t kind;   // KMV_*
  uint8_t* plane;  // n_slots + 1 entries of 8 / 16 bytes
  uint8_t* valid;  // n_slots + 1 bytes
};

__device__ __forceinline__ void key_map_store_values(const KeptRows& rows, const FilterRow& r, const KeyMapValueJob* vals, uint32_t n_values, uint32_t n_cols, uint32_t at) {
  for (uint32_t k = 0; k < n_values; k++) {
    const KeyMapValueJob v = vals[k];
    if (v.col >= n_cols) continue;
    const FilterCol c = rows.cols[v.col];
    const bool ok = filter_valid(c, r.u, r.l, rows.W);
    if (v.kind == KMV_DEC128) {
      uint4 q = {0, 0, 0, 0};
      if (ok) q = reinterpret_cast<const uint4*>(c.values)[r.row];
      reinterpret_cast<uint4*>(v.plane)[at] = q;
    } else if (v.kind == KMV_F64) {
      reinterpret_cast<double*>(v.plane)[at] = ok ? filter_load_f64(c, r.row) : 0.0;
    } else {
      reinterpret_cast<long long*>(v.plane)[at] = ok ? filter_load_i64(c, r.row) : 0ll;
    }
    v.valid[at] = ok ? 1 : 0;
  }
}

// Resource usage (gfx950): 37 VGPRs, 106 SGPRs (20 SGPRs spilled to VGPR lanes, none to memory), no scratch, 16 bytes of LDS;
// occupancy 7 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
key_map_insert_kernel(KeptRows rows, uint32_t n_cols, uint32_t col, unsigned long long* slots, uint32_t n_slots, uint32_t max_keys, uint32_t hash_mask, KeySetControl* ctl,
                      const KeyMapValueJob* vals, uint32_t n_values) {
  __shared__ uint32_t new_s[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, mask = n_slots - 1;
  const FilterCol c = rows.cols[col];
  const FilterWords ws = filter_words(rows.n_in);
  if (n_values > kKeyMapMaxValues) n_values = kKeyMapMaxValues;
  uint32_t n_new = 0;  // (wave-uniform: popcounts of ballots)
  bool has_null = false, full = false, dup = false;
  for (uint64_t w = ws.first; w < ws.n; w += ws.stride) {
    if (__atomic_load_n(&ctl->flags, __ATOMIC_RELAXED) & KEY_SET_OVERFLOW) break;  // (the map is refused: nothing more goes in)
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
      uint32_t at = n_slots;  // (the sentinel's value: the planes' extra entry)
      if (key == kKeySetSentinel) {
        is_new = !(atomicOr(&ctl->flags, (uint32_t)KEY_SET_HAS_SENTINEL) & KEY_SET_HAS_SENTINEL);
        dup = dup || !is_new;
      } else {
        bool done = false;
        uint32_t s = in_first_slot(in_hash_i64(key), hash_mask, mask);
        for (uint32_t step = 0; step < n_slots && !done; step++, s = (s + 1) & mask) {
          if ((step & 1023) == 1023 && (__atomic_load_n(&ctl->flags, __ATOMIC_RELAXED) & KEY_SET_OVERFLOW)) {
            done = true;  // (refused meanwhile: the key is dropped with the map)
            break;
          }
          unsigned long long cur = __atomic_load_n(&slots[s], __ATOMIC_RELAXED);
          if (cur == kKeySetSentinel) {
            cur = atomicCAS(&slots[s], kKeySetSentinel, key);
            if (cur == kKeySetSentinel) {
              is_new = true;
              done = true;
              at = s;
            }
          }
          if (cur == key) {  // (never after a claim: cur is the sentinel then, which is not the key)
            dup = true;
            done = true;
          }
        }
        full = full || !done;  // (n_slots steps, neither the key nor a free slot: more than max_keys keys are in)
      }
      if (is_new) key_map_store_values(rows, r, vals, n_values, n_cols, at);
    }
    n_new += (uint32_t)__builtin_popcountll(__ballot(is_new));
  }
  if (__ballot(full) && lane == 0) atomicOr(&ctl->flags, (uint32_t)KEY_SET_OVERFLOW);
  if (__ballot(dup) && lane == 0) atomicOr(&ctl->flags, (uint32_t)KEY_MAP_DUPLICATE);
  if (__ballot(has_null) && lane == 0 && !(__atomic_load_n(&ctl->flags, __ATOMIC_RELAXED) & KEY_SET_HAS_NULL)) atomicOr(&ctl->flags, (uint32_t)KEY_SET_HAS_NULL);
  if (lane == 0) new_s[wave] = n_new;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t n = new_s[0] + new_s[1] + new_s[2] + new_s[3];
    if (n && atomicAdd(&ctl->n_keys, n) + n > max_keys) atomicOr(&ctl->flags, (uint32_t)KEY_SET_OVERFLOW);
  }
}

// One value column of a probe
struct LookupValueJob {
  const uint8_t* plane;              // the map's value plane: n_slots + 1 entries of `width` bytes
  const uint8_t* valid;              // ... and its validity bytes
  uint8_t* out_values;               // n_rows values of `width` bytes
  unsigned long long* out_validity;  // n_batches * W words
  unsigned long long* null_counts;   // n_batches counts, zero before the launch
  uint32_t width;                    // 8 or 16
  uint32_t pad;
};
// One (map, probe key column) pair of one stripe
struct LookupJob {
  FilterCol key;         // the probe key column as the decode left it (FKIND_INT)
  const uint8_t* table;  // the map's sealed table: header, occupancy, slots
  uint32_t table_bytes;
  uint32_t n_slots;      // the host's: the planes hold n_slots + 1 entries
  uint32_t n_values;     // 1 .. 8
  uint32_t pad;
  LookupValueJob v[kKeyMapMaxValues];
};

// Resource usage (gfx950): 20 VGPRs, 29 SGPRs, no scratch (none expected, none used), no spill, 32768 bytes of LDS (the staged table);
// occupancy 5 waves / SIMD, which the LDS sets: five 32 KiB blocks share a CU's 160 KiB.
__global__ __launch_bounds__(256) void lookup_columns_kernel(const LookupJob* jobs, uint64_t n_rows, uint32_t n_batches, uint32_t B, uint32_t W) {
  __shared__ unsigned long long tab_s[kInLdsBytes / 8];
  const LookupJob* job = jobs + blockIdx.y;
  const uint32_t bytes = job->table_bytes & ~7u;
  const uint8_t* tab = job->table;
  if (bytes >= kInHeaderBytes && bytes <= kInLdsBytes) {  // (uniform over the block; every wavefront reaches the barrier)
    const unsigned long long* g8 = reinterpret_cast<const unsigned long long*>(job->table);
    for (uint32_t x = threadIdx.x; x < bytes / 8; x += 256) tab_s[x] = g8[x];
    __syncthreads();
    tab = reinterpret_cast<const uint8_t*>(tab_s);
  }
  const uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= (uint64_t)n_batches * W) return;  // (the whole wavefront: the ballots below are taken by the wavefronts that stay)
  InTable t = in_table(tab, bytes < kInHeaderBytes ? 0 : bytes);
  const uint32_t n_slots = job->n_slots;
  if (t.kind != IN_KEY_I64 || t.n_slots != n_slots) t.n_slots = 0;  // (not the table the planes were laid out for: nothing matches)
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t u = g / W;
  const uint32_t l = (uint32_t)(g % W) * 64 + lane;
  const uint64_t row = u * B + l;
  const bool live = l < B && row < n_rows;
  uint32_t at = kKeyMapNoSlot;
  if (live && t.n_slots && filter_valid(job->key, u, l, W)) {
    const unsigned long long key = (unsigned long long)filter_load_i64(job->key, row);
    const uint32_t s = in_find_i64(t, key);
    if (s != kKeyMapNoSlot) at = key_map_value_index(s, key, n_slots);
  }
  const unsigned long long m_live = __ballot(live);
  const uint32_t nv = job->n_values < kKeyMapMaxValues ? job->n_values : kKeyMapMaxValues;
  for (uint32_t k = 0; k < nv; k++) {
    const LookupValueJob* v = job->v + k;
    const bool valid = at != kKeyMapNoSlot && v->valid[at] != 0;
    if (live) {
      if (v->width == 16) {
        uint4 q = {0, 0, 0, 0};
        if (valid) q = reinterpret_cast<const uint4*>(v->plane)[at];
        reinterpret_cast<uint4*>(v->out_values)[row] = q;
      } else {
        reinterpret_cast<unsigned long long*>(v->out_values)[row] = valid ? reinterpret_cast<const unsigned long long*>(v->plane)[at] : 0ull;
      }
    }
    const unsigned long long m_valid = __ballot(valid);
    if (lane == 0) {
      v->out_validity[g] = m_valid;
      const uint32_t nulls = (uint32_t)(__popcll(m_live) - __popcll(m_valid));
      if (nulls) atomicAdd(v->null_counts + u, (unsigned long long)nulls);
    }
  }
}
