// agg_group_kernels.hip -- GROUP BY for the aggregates of agg_kernels.hip: the kept rows of a decoded stripe reduced to one
// record per (aggregate, group), for at most kGroupMax (256) groups a stripe.  Nothing is sorted, gathered or copied back but the
// groups' keys and records.  The semantics are those of include/orcgpu.h (orcgpu_result_aggregate_groups).
//
//   group_assign_kernel       over the words of the keep mask, like agg_partial_kernel.  A kept row hashes its key tuple (per key
//                             the validity bit and the int64 / 128-bit value / string bytes) and probes an open-addressing table
//                             of kGroupSlots slots in global memory, linear probing.  A free slot is claimed with a 64-bit
//                             atomicCAS that stores the claiming input row + 1; a claimed one is compared by loading its claimer's
//                             keys through the row-access layer (filter_access.h): there is no second copy of the keys.  The row's
//                             slot goes to a uint32 plane, one entry per input row, and the slot's smallest row is kept with an
//                             atomicMax on ~row -- once per (wavefront, slot) and only while it still raises the value.  More
//                             than kGroupMax claims set GROUP_TOO_MANY; later rows stop inserting.
//   group_number_kernel       one block of kGroupSlots threads: ranks the claimed slots by their first row -> the dense group
//                             number of every slot and n_groups, and a GroupKeyRecord per (group, key) from the first row.  Which
//                             row won which slot cannot show: numbers, keys and order come from the first rows alone.
//   agg_group_partial_kernel  grid (agg_group_blocks(n_in), instructions).  Every wavefront owns a table of kGroupMax AggAcc in
//                             LDS.  Per 64-row word a lane loads its row as agg_partial_kernel does (agg_row) into an accumulator
//                             of one row; the wavefront folds the lanes of one group into acc[group] in a fixed order (below).
//                             Behind the last trip thread t folds acc[t] of the four wavefronts in wavefront order and stores the
//                             record (instruction, block, group t).
//   agg_group_final_kernel    one block per (group, instruction): the blocks' records in index order, agg_final_kernel's tree.
//
// The fold of a word into LDS, by the number of distinct groups d among its kept lanes -- a function of the data alone, so the same
// call takes the same path and a Float sum keeps its bits:
//   d <= kGroupTreeMax (4)    per distinct group, lowest lane first, a masked agg_wave_fold (the lanes of other groups hold the
//                             empty accumulator) and lane 0 folds the result into acc[group]: 6 shuffle steps a group, whatever the
//                             multiplicity.  The Q1 kind: a handful of flags.
//   else                      rounds: a lane's rank among the lanes of its group (popcount of the ballot below it) picks the round
//                             in which it folds its row into acc[group]; the lanes of a round hold different groups, so different
//                             addresses.  As many rounds as the largest multiplicity, at most 64 / d rounded up when spread evenly.
// The threshold is reasoned, not tuned: a tree step moves six 64-bit values by shuffle, a round is one 48-byte LDS read-modify-write,
// and for d groups spread evenly the two cost 6 d steps against 64 / d rounds.
//
// LDS: 4 x 256 x 48 B = 48 KiB a block (three blocks a CU of 160 KiB).  acc[group] is 48 bytes wide, 12 banks: lanes of one round
// on groups 16 apart (b64 accesses, 64 banks) share banks -- up to 4-way, on the rounds path and in the last fold only.
// No floating-point atomic anywhere; the integer atomics (CAS, Max, Add, Or) decide slots and flags, never a value handed out.
//
// Resource usage of the two wide kernels (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): in front of each.
#pragma once
#include <stdint.h>

#include "agg_group_program.h"
#include "agg_kernels.hip"

constexpr uint32_t kGroupTreeMax = 4;

// ---- a row's key tuple: its hash, and whether two rows hold the same ----
__device__ __forceinline__ unsigned long long group_key_hash(const FilterCol& c, uint32_t fkind, const FilterRow& r, uint32_t B, uint32_t W) {
  if (!filter_valid(c, r.u, r.l, W)) return 0x9e3779b97f4a7c15ull;  // NULL: a key value of its own
  switch (fkind) {
    case FKIND_BOOL: return 2 + (unsigned long long)filter_load_bit(c, r.u, r.l, W);
    case FKIND_DEC128: {
      unsigned long long lo, hi;
      filter_load_dec128(c, r.row, &lo, &hi);
      return 4 + (unsigned long long)in_hash_dec128(lo, hi);
    }
    case FKIND_STRING: {
      const FilterStr s = filter_value_str(c, r.u, r.l, B);
      return 4 + (unsigned long long)in_hash_bytes(s.p, s.len);
    }
    default: return 4 + in_mix64((unsigned long long)filter_load_i64(c, r.row));
  }
}
__device__ __forceinline__ uint32_t group_row_hash(const GroupKeys& keys, const FilterCol* cols, const FilterRow& r, uint32_t B, uint32_t W) {
  unsigned long long h = 0;
  for (uint32_t k = 0; k < keys.n; k++) h = in_mix64(h + group_key_hash(cols[keys.col[k]], keys.fkind[k], r, B, W) + k);
  return (uint32_t)h & keys.hash_mask;
}
__device__ __forceinline__ bool group_key_equal(const FilterCol& c, uint32_t fkind, const FilterRow& a, const FilterRow& b, uint32_t B, uint32_t W) {
  const bool va = filter_valid(c, a.u, a.l, W), vb = filter_valid(c, b.u, b.l, W);
  if (!va || !vb) return va == vb;
  switch (fkind) {
    case FKIND_BOOL: return filter_load_bit(c, a.u, a.l, W) == filter_load_bit(c, b.u, b.l, W);
    case FKIND_DEC128: {
      unsigned long long alo, ahi, blo, bhi;
      filter_load_dec128(c, a.row, &alo, &ahi);
      filter_load_dec128(c, b.row, &blo, &bhi);
      return alo == blo && ahi == bhi;
    }
    case FKIND_STRING: {
      const FilterStr x = filter_value_str(c, a.u, a.l, B), y = filter_value_str(c, b.u, b.l, B);
      if (x.len != y.len) return false;
      for (uint32_t k = 0; k < x.len; k++)
        if (x.p[k] != y.p[k]) return false;
      return true;
    }
    default: return filter_load_i64(c, a.row) == filter_load_i64(c, b.row);
  }
}
__device__ __forceinline__ bool group_rows_equal(const GroupKeys& keys, const FilterCol* cols, const FilterRow& a, const FilterRow& b, uint32_t B, uint32_t W) {
  for (uint32_t k = 0; k < keys.n; k++)
    if (!group_key_equal(cols[keys.col[k]], keys.fkind[k], a, b, B, W)) return false;
  return true;
}

// table (kGroupSlots slots) and ctl are zeroed by the call before this kernel; plane gets one entry per input row of the words
// that hold a kept row: the row's slot, or kGroupNoSlot for a row that is not kept or stopped inserting.  Every index into the
// table is masked to kGroupSlots; a claimer read from a slot is an input row some thread put there, so below n_in.
// (The body of two kernels: group_assign_kernel gives it the constants kGroupSlots and kGroupMax, group_wide_assign_kernel of
// agg_group_wide_kernels.hip a table of `slots` slots -- a power of two -- and the limit `max_groups` that was set.)
__device__ __forceinline__ void group_assign_body(const GroupKeys& keys, const KeptRows& rows, GroupSlot* table, const uint32_t slots, const uint32_t max_groups,
                                                  GroupControl* ctl, uint32_t* plane) {
  const uint32_t lane = threadIdx.x & 63;
  const FilterCol* const cols = rows.cols;
  const uint64_t n_in = rows.n_in;
  const uint32_t B = rows.B, W = rows.W;
  const FilterWords ws = filter_words(n_in);
  for (uint64_t w = ws.first; w < ws.n; w += ws.stride) {
    const unsigned long long m = agg_keep_word(rows, w);
    if (!m) continue;
    const uint64_t j = w * 64 + lane;
    const bool kept = ((m >> lane) & 1) && j < n_in;
    uint32_t slot = kGroupNoSlot;
    if (kept) {
      const FilterRow r = filter_row(rows, j);
      const uint32_t h = group_row_hash(keys, cols, r, B, W);
      for (uint32_t step = 0; step < slots; step++) {
        const uint32_t s = (h + step) & (slots - 1);
        unsigned long long cur = __atomic_load_n(&table[s].claim, __ATOMIC_RELAXED);
        if (!cur) {
          if (__atomic_load_n(&ctl->flags, __ATOMIC_RELAXED) & GROUP_TOO_MANY) break;  // (the answer is refused: nothing more goes in)
          cur = atomicCAS(&table[s].claim, 0ull, (unsigned long long)(j + 1));
          if (!cur) {
            if (atomicAdd(&ctl->claimed, 1u) >= max_groups) atomicOr(&ctl->flags, (uint32_t)GROUP_TOO_MANY);
            slot = s;
            break;
          }
        }
        const uint64_t rep = cur - 1;
        if (rep == j || (rep < n_in && group_rows_equal(keys, cols, r, filter_row(rows, rep), B, W))) {
          slot = s;
          break;
        }
      }
      if (slot == kGroupNoSlot) atomicOr(&ctl->flags, (uint32_t)GROUP_TOO_MANY);  // (stopped, or the table is full: more than kGroupMax claims)
    }
    plane[j] = slot;  // (the plane holds 64 entries for every word of the mask)
    // the slot's first row: the lowest lane of every slot in this word speaks for the others, and only while it lowers the row
    unsigned long long todo = __ballot(slot != kGroupNoSlot);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const uint32_t ls = (uint32_t)__shfl((int)slot, leader);
      const unsigned long long same = __ballot(slot == ls);
      if ((int)lane == leader && __atomic_load_n(&table[ls].first_inv, __ATOMIC_RELAXED) < ~j) atomicMax(&table[ls].first_inv, ~j);
      todo &= ~same;
    }
  }
}
// Resource usage (gfx950): 62 VGPRs, 105 SGPRs, no scratch, no spill, no LDS; occupancy 7 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
group_assign_kernel(GroupKeys keys, KeptRows rows, GroupSlot* table, GroupControl* ctl, uint32_t* plane) {
  group_assign_body(keys, rows, table, kGroupSlots, kGroupMax, ctl, plane);
}

// The GroupKeyRecord of every key column of group `rank`, from the group's first row `first` (an input row below n_in) ->
// key_recs[rank][key]; a String key of more than kGroupKeyBytes bytes sets the key's flag
__device__ __forceinline__ void group_store_keys(const GroupKeys& keys, const KeptRows& rows, uint64_t first, uint32_t rank, GroupControl* ctl, GroupKeyRecord* key_recs) {
  const uint32_t B = rows.B, W = rows.W;
  const FilterRow r = filter_row(rows, first);
  for (uint32_t k = 0; k < keys.n; k++) {
    const FilterCol c = rows.cols[keys.col[k]];
    GroupKeyRecord* out = key_recs + (uint64_t)rank * keys.n + k;
    out->is_null = 0;
    out->len = 0;
    out->w[0] = out->w[1] = 0;
    for (uint32_t x = 0; x < kGroupKeyBytes; x++) out->bytes[x] = 0;
    if (!filter_valid(c, r.u, r.l, W)) {
      out->is_null = 1;
      continue;
    }
    if (keys.fkind[k] == FKIND_BOOL) {
      out->w[0] = filter_load_bit(c, r.u, r.l, W);
    } else if (keys.fkind[k] == FKIND_DEC128) {
      unsigned long long lo, hi;
      filter_load_dec128(c, r.row, &lo, &hi);
      out->w[0] = lo;
      out->w[1] = hi;
    } else if (keys.fkind[k] == FKIND_STRING) {
      const FilterStr v = filter_value_str(c, r.u, r.l, B);
      out->len = v.len;
      if (v.len > kGroupKeyBytes) atomicOr(&ctl->flags, (uint32_t)GROUP_KEY_TOO_LONG << k);
      for (uint32_t x = 0; x < v.len && x < kGroupKeyBytes; x++) out->bytes[x] = v.p[x];
    } else {
      const long long v = filter_load_i64(c, r.row);
      out->w[0] = (unsigned long long)v;
      out->w[1] = (unsigned long long)(v >> 63);
    }
  }
}

// <<<1, kGroupSlots>>>: thread s is slot s.  slot_group[s] = the slot's dense group number (kGroupNoSlot: free, or past kGroupMax);
// key_recs: [group][key].  Nothing is numbered for a table that holds more than kGroupMax groups.
extern "C" __global__ void __launch_bounds__(1024)
group_number_kernel(GroupKeys keys, KeptRows rows, const GroupSlot* table, GroupControl* ctl, uint32_t* slot_group, GroupKeyRecord* key_recs) {
  __shared__ unsigned long long first_s[kGroupSlots];
  __shared__ uint32_t n_s;
  const uint32_t s = threadIdx.x;
  if (s == 0) n_s = 0;
  const bool used = table[s].claim != 0;
  const unsigned long long first = used ? ~table[s].first_inv : ~0ull;
  first_s[s] = first;
  __syncthreads();
  uint32_t rank = 0;
  if (used) {
    for (uint32_t t = 0; t < kGroupSlots; t++) rank += first_s[t] < first;
    atomicAdd(&n_s, 1u);
  }
  __syncthreads();
  const uint32_t n_groups = n_s;
  const bool fits = n_groups <= kGroupMax && !(ctl->flags & GROUP_TOO_MANY);
  if (s == 0) {
    ctl->n_groups = n_groups;
    if (n_groups > kGroupMax) atomicOr(&ctl->flags, (uint32_t)GROUP_TOO_MANY);
  }
  const bool mine = used && fits && rank < kGroupMax && first < rows.n_in;
  slot_group[s] = mine ? rank : kGroupNoSlot;
  if (mine) group_store_keys(keys, rows, first, rank, ctl, key_recs);
}

// partials: [instruction][block][group], kGroupMax groups a block of which the first ctl->n_groups are written.  The plane's
// entries are trusted no further than a slot index below kGroupSlots, the numbers of slot_group no further than a group below
// kGroupMax: whatever a refused table left in them, every LDS and global address stays in bounds.
// Resource usage (gfx950): agg_group_partial_kernel 70 VGPRs, 106 SGPRs; agg_group_expr_partial_kernel 75 VGPRs, 106 SGPRs
// (agg_group_expr_div_partial_kernel, with the divide: 85 VGPRs); all no scratch, no
// spill of either register kind, 49152 bytes of LDS: three blocks a CU by LDS, 3 waves / SIMD.  (The condition's word is ONE scalar load
// a trip, cond[w]: a lane's bit of its own word, loaded per lane, cost two and four scalar registers spilled to VGPR lanes.)
// A kept row whose instruction has a condition (AggInsn::cond) and does not pass it is a lane that holds the empty contribution: it
// keeps its group, its rank and its place in the tree or the rounds, so the condition never changes which shape runs.
// (The body of two kernels: EXPR = false is agg_group_partial_kernel, which takes the plain kinds and leaves the AK_EXPR_* rows of
// grid.y at once; EXPR = true is agg_group_expr_partial_kernel, the other way round, launched only when the list holds such an
// instruction -- the interpreter's registers are not the plain kinds'.  ops: the op table of the programs, EXPR only.  DIV: the
// interpreter with the divide, agg_group_expr_div_partial_kernel, launched in its place when a program holds a division.)
template <bool EXPR, bool DIV = false, bool COND = false, bool CONV = false>
__device__ __forceinline__ void agg_group_partial_body(const AggInsn* insns, const AggExprOp* ops, const KeptRows& rows, const uint32_t* plane,
                                                       const uint32_t* slot_group, const GroupControl* ctl, AggPartial* partials, AggAcc (*acc_s)[kGroupMax]) {
  const FilterCol* const cols = rows.cols;
  const uint64_t n_in = rows.n_in;
  const uint32_t W = rows.W;
  if (ctl->flags & GROUP_TOO_MANY) return;  // (uniform: the whole grid leaves)
  const uint32_t n_groups = ctl->n_groups < kGroupMax ? ctl->n_groups : kGroupMax;
  const AggInsn in = insns[blockIdx.y];
  if (agg_is_expr(in.kind) != EXPR) return;  // (uniform over the block)
  const uint32_t kind = EXPR ? in.kind : in.kind < AK_N ? in.kind : AK_COUNT_ROWS;
  const bool is_max = in.is_max != 0;
  const FilterCol c = cols[EXPR ? 0 : in.col], c2 = cols[EXPR ? 0 : in.col2];  // (EXPR: col / col2 are no column indexes; unused)
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const AggAcc zero = {0, 0, 0, 0.0, 0, 0};
  bool blocked;
  const unsigned long long* const cond = agg_cond_plane(rows, in.cond, &blocked);
  AggAcc* const acc = acc_s[wave];
  for (uint32_t g = lane; g < kGroupMax; g += 64) acc[g] = zero;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  const FilterWords ws = filter_words(n_in);
  for (uint64_t w = ws.first; w < ws.n; w += ws.stride) {
    const unsigned long long m = agg_keep_word(rows, w);
    if (!m) continue;
    const uint64_t j = w * 64 + lane;
    uint32_t g = kGroupNoSlot;
    AggAcc v = zero;
    if (((m >> lane) & 1) && j < n_in) {
      const uint32_t slot = plane[j];
      g = slot < kGroupSlots ? slot_group[slot] : kGroupNoSlot;
      if (g >= n_groups) g = kGroupNoSlot;
    }
    const bool kept = g != kGroupNoSlot;
    // (a row its instruction's condition does not pass keeps the empty contribution and its place in the fold below)
    const unsigned long long pass_m = blocked ? 0ull : cond ? cond[w] : ~0ull;  // (the word's rows that pass: one scalar load a word)
    if (kept && ((pass_m >> lane) & 1)) {
      if constexpr (EXPR) agg_expr_row<DIV, COND, CONV>(kind, ops + in.col, in.col2, cols, filter_row(rows, j), W, v);
      else if (kind == AK_COUNT_ROWS) v.w0 = 1;
      else agg_row(kind, is_max, in, c, c2, filter_row(rows, j), W, v);
    }
    // the distinct groups of the word, and a lane's peers: the lanes that hold its group
    unsigned long long todo = __ballot(kept), peers = 0;
    uint32_t d = 0;
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const uint32_t lg = (uint32_t)__shfl((int)g, leader);
      const unsigned long long same = __ballot(kept && g == lg);
      if (kept && g == lg) peers = same;
      todo &= ~same;
      d++;
    }
    if (!d) continue;
    if (d <= kGroupTreeMax) {
      todo = __ballot(kept);
      while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lg = (uint32_t)__shfl((int)g, leader);
        const bool in_it = kept && g == lg;
        AggAcc t = in_it ? v : zero;
        agg_wave_fold(kind, is_max, t);
        if (lane == 0) {
          AggAcc a = acc[lg];
          agg_fold(kind, is_max, a, t);
          acc[lg] = a;
        }
        todo &= ~__ballot(in_it);
      }
    } else {
      const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
      uint32_t rounds = kept ? (uint32_t)__popcll(peers) : 0;
      for (int o = 32; o; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)rounds, o);
        rounds = other > rounds ? other : rounds;
      }
      for (uint32_t round = 0; round < rounds; round++) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // (a round reads what the round before wrote, from another lane)
        if (kept && rank == round) {
          AggAcc a = acc[g];
          agg_fold(kind, is_max, a, v);
          acc[g] = a;
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  __syncthreads();
  const uint32_t t = threadIdx.x;
  if (t < n_groups) {
    AggAcc a = acc_s[0][t];
    for (uint32_t x = 1; x < 4; x++) agg_fold(kind, is_max, a, acc_s[x][t]);
    agg_store(partials + ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * kGroupMax + t, a);
  }
}
extern "C" __global__ void __launch_bounds__(256)
agg_group_partial_kernel(const AggInsn* insns, KeptRows rows, const uint32_t* plane, const uint32_t* slot_group, const GroupControl* ctl, AggPartial* partials) {
  __shared__ AggAcc acc_s[4][kGroupMax];
  agg_group_partial_body<false>(insns, nullptr, rows, plane, slot_group, ctl, partials, acc_s);
}
extern "C" __global__ void __launch_bounds__(256)
agg_group_expr_partial_kernel(const AggInsn* insns, const AggExprOp* ops, KeptRows rows, const uint32_t* plane, const uint32_t* slot_group, const GroupControl* ctl,
                              AggPartial* partials) {
  __shared__ AggAcc acc_s[4][kGroupMax];
  agg_group_partial_body<true>(insns, ops, rows, plane, slot_group, ctl, partials, acc_s);
}
extern "C" __global__ void __launch_bounds__(256)
agg_group_expr_div_partial_kernel(const AggInsn* insns, const AggExprOp* ops, KeptRows rows, const uint32_t* plane, const uint32_t* slot_group, const GroupControl* ctl,
                                  AggPartial* partials) {
  __shared__ AggAcc acc_s[4][kGroupMax];
  agg_group_partial_body<true, true>(insns, ops, rows, plane, slot_group, ctl, partials, acc_s);
}
// (the interpreter with the divide and the conditionals: launched when a program of the list holds a conditional op)
extern "C" __global__ void __launch_bounds__(256)
agg_group_expr_cond_partial_kernel(const AggInsn* insns, const AggExprOp* ops, KeptRows rows, const uint32_t* plane, const uint32_t* slot_group, const GroupControl* ctl,
                                   AggPartial* partials) {
  __shared__ AggAcc acc_s[4][kGroupMax];
  agg_group_partial_body<true, true, true>(insns, ops, rows, plane, slot_group, ctl, partials, acc_s);
}
// (the mixed interpreter: launched when a program of the list holds a conversion)
extern "C" __global__ void __launch_bounds__(256)
agg_group_expr_conv_partial_kernel(const AggInsn* insns, const AggExprOp* ops, KeptRows rows, const uint32_t* plane, const uint32_t* slot_group, const GroupControl* ctl,
                                   AggPartial* partials) {
  __shared__ AggAcc acc_s[4][kGroupMax];
  agg_group_partial_body<true, true, true, true>(insns, ops, rows, plane, slot_group, ctl, partials, acc_s);
}

// grid (kGroupMax, instructions): block (g, k) folds the n_blocks records of group g under instruction k -> out[k][g]; the blocks
// of groups that do not exist leave at once
extern "C" __global__ void __launch_bounds__(256)
agg_group_final_kernel(const AggInsn* insns, const AggPartial* partials, uint32_t n_blocks, const GroupControl* ctl, AggPartial* out) {
  __shared__ AggAcc fold_s[4];
  if ((ctl->flags & GROUP_TOO_MANY) || blockIdx.x >= ctl->n_groups) return;
  const AggInsn in = insns[blockIdx.y];
  const uint32_t kind = in.kind < AK_ALL_N ? in.kind : AK_COUNT_ROWS;
  const AggAcc a = agg_fold_records(kind, in.is_max != 0, partials + (uint64_t)blockIdx.y * n_blocks * kGroupMax + blockIdx.x, kGroupMax, n_blocks, fold_s);
  if (threadIdx.x == 0) agg_store(out + (uint64_t)blockIdx.y * kGroupMax + blockIdx.x, a);
}
