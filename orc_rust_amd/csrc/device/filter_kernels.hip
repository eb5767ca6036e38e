// filter_kernels.hip -- a ROW FILTER over a decoded stripe: per-row predicate evaluation and a compacting gather.
//
// The reference has no row-level evaluation (its predicates prune row groups only, row_group_filter.rs); the semantics are
// those of include/orcgpu.h (orcgpu_result_filter): SQL three-valued logic, a row is kept when the root is TRUE.
//
//   filter_eval_kernel    one lane per input row, one 64-bit word of the keep mask per wavefront trip.  The predicate is a
//                         post-order program (FilterInsn); a leaf yields two ballot words for the trip's 64 rows -- the rows
//                         where it is TRUE and the rows where it is FALSE (neither: UNKNOWN) --, inner nodes combine words on
//                         a per-wavefront stack with wave-uniform code.  Writes keep = T_root & live and its popcount.
//                         A Decimal leaf compares the row's 16 bytes with a literal the host has brought to the column's scale,
//                         a Timestamp leaf is the integer leaf on a literal in the column's unit: no row is ever rescaled.
//                         The evaluation of one word is filter_eval_word, which the aggregates' conditions run too
//                         (agg_cond_eval_kernel, agg_kernels.hip).
//   filter_like_kernel    runs in front of it when the program holds LIKE leaves: per leaf a plane of match bits, one word per
//                         64 input rows like `keep`; the evaluation forms T = match & valid, F = ~match & valid from it.  The
//                         compiled pattern (parts of literal bytes and `_` marks between the `%`) lies in LDS; no backtracking;
//                         a lane per short value, the wavefront on 64 candidate starts at once for a long one.
//   filter_in_kernel      likewise for IN leaves: per leaf a plane of "the row is valid and its key is in the list", from a hash
//                         set the host has built (filter_program.h): staged in LDS up to 32 KiB, probed in global memory above;
//                         a lane per value, so a row costs one probe however long the list is.  A set leaf (FOP_IN_SET) is the
//                         same leaf against a table key_set_seal_kernel left in that layout (key_set_kernels.hip).
//   filter_expr_kernel    likewise for expression leaves (lhs OP rhs): per leaf TWO planes, the rows where the comparison is TRUE
//                         and the rows where it is FALSE (neither: UNKNOWN -- a NULL column on either side, or an operation inside
//                         a side that left 128 bits, which it counts).  A lane per row interprets both sides' op tables
//                         (agg_expr_eval.h, the expression aggregates' evaluator) and compares (filter_expr_eval.h).
//   (enc_scan)            exclusive scan of the popcounts: the output row of every word's first kept row.
//   filter_place_kernel   every kept row writes its stripe row at its output row: src_rows[], the gather's index list.
//   filter_count_kernel   per (output batch, column): null count and string bytes -- what the host needs to lay the output out
//                         compactly; it is fetched with the row count in the filter's ONE host wait.
//   filter_gather_kernel  per (output batch, column): fixed-width values (16-byte stores where the batch's first value is
//                         16-byte aligned), Boolean bits and validity rebuilt by ballot, string lengths -> offsets restarting
//                         at 0 (a block scan) -> bytes (a lane per short value, a wavefront per long one).
//
// The input rows are the result's rows as its batches hand them out: all rows of the stripe (n_segs = 0), or the row ranges
// of a row selection (SelBatch segments).  Leaves and the gather read the stripe-wide buffers of the decode the way
// select_build_kernel does: uniform batches of `B` rows, `W` validity words per batch, string offsets that restart per
// batch plus the batch's char base.  Output rows [k * B, (k + 1) * B) form output batch k.  All of that is written down once, in
// the row-access helpers of filter_access.h (filter_row .. filter_value_str), which the aggregation kernels share: a kernel
// addresses a row through them only.
#pragma once
#include <stdint.h>

#include "filter_program.h"
#include "filter_access.h"
#include "filter_expr_eval.h"

struct FilterGatherJob {
  FilterCol src;
  unsigned long long* out_validity;           // per output batch W words (null: the kept rows hold no null)
  uint8_t* out_values;                        // fixed width: output row * width; Boolean: W words per output batch
  int32_t* out_offsets;                       // strings: per output batch B + 1
  uint8_t* out_chars;                         // strings: the kept rows' bytes, batch after batch
  const unsigned long long* out_char_base;    // strings: per output batch, where its bytes start in out_chars
};

constexpr uint32_t kFilterShortString = 32;    // values up to this many bytes are copied by one lane, longer ones by a wavefront

// Leaf blockIdx.y of a plane kernel's leaf list: its instruction.  false -- the whole block leaves -- for what only a damaged
// upload holds: an index past the program, an instruction of another op, a plane past the workspace's.
// (op_too: a second op the list may hold -- filter_in_kernel's list holds FOP_IN and FOP_IN_SET leaves)
__device__ __forceinline__ bool filter_leaf(const FilterInsn* prog, uint32_t n_insn, const uint32_t* leaves, uint32_t op, uint32_t n_planes,
                                            FilterInsn* in, uint32_t op_too = ~0u) {
  const uint32_t k = leaves[blockIdx.y];
  if (k >= n_insn) return false;
  *in = prog[k];
  return (in->op == op || in->op == op_too) && (unsigned long long)in->i < n_planes;
}

// ---- LIKE: the compiled pattern of filter_program.h, staged in LDS ----
struct LikePat {
  uint32_t shape, flags, n_parts, n_elems;
  const uint32_t* parts;  // per part {first element, elements}
  const uint8_t* bytes;   // per element: the literal byte
  const uint8_t* ones;    // per element: 1 = `_`
};
constexpr uint32_t kLikeFail = 0xffffffffu;

// Part [first, first + n) matched forwards from position s of the value p[0, end): where the match ends, or kLikeFail.  A `_`
// takes the byte that stands there and the continuation bytes behind it.  Nothing at or behind `end` is loaded.
template <bool LIT>
__device__ __forceinline__ uint32_t like_fwd(const uint8_t* p, uint32_t s, uint32_t end, const LikePat& P, uint32_t first, uint32_t n) {
  uint32_t q = s;
  for (uint32_t k = 0; k < n; k++) {
    if (q >= end) return kLikeFail;
    if (!LIT && P.ones[first + k]) {
      q++;
      while (q < end && (p[q] & 0xC0) == 0x80) q++;
    } else {
      if (p[q] != P.bytes[first + k]) return kLikeFail;
      q++;
    }
  }
  return q;
}
// ... and backwards from `e`, where the match is to end, without stepping below `lo`: where the match starts, or kLikeFail
template <bool LIT>
__device__ __forceinline__ uint32_t like_bwd(const uint8_t* p, uint32_t lo, uint32_t e, const LikePat& P, uint32_t first, uint32_t n) {
  uint32_t q = e;
  for (uint32_t k = n; k-- > 0;) {
    if (q <= lo) return kLikeFail;
    q--;
    if (!LIT && P.ones[first + k]) {
      while (q > lo && (p[q] & 0xC0) == 0x80) q--;
    } else if (p[q] != P.bytes[first + k]) return kLikeFail;
  }
  return q;
}
// The leftmost match of a part that starts in [pos, end - n]: where it ends, or kLikeFail.  One lane walks the starts one by one;
// a wavefront (every lane with the same value) tests 64 starts at once and takes the first hit by ballot.
template <bool WAVE, bool LIT>
__device__ __forceinline__ uint32_t like_find(const uint8_t* p, uint32_t pos, uint32_t end, const LikePat& P, uint32_t first, uint32_t n, uint32_t lane) {
  if (end - pos < n) return kLikeFail;
  const uint32_t last = end - n;  // (every element takes a byte at least)
  if (!WAVE) {
    for (uint32_t s = pos; s <= last; s++) {
      const uint32_t q = like_fwd<LIT>(p, s, end, P, first, n);
      if (q != kLikeFail) return q;
    }
    return kLikeFail;
  }
  for (uint32_t base = pos; base <= last; base += 64) {
    const uint32_t s = base + lane;
    const uint32_t q = s <= last ? like_fwd<LIT>(p, s, end, P, first, n) : kLikeFail;
    const unsigned long long hit = __ballot(q != kLikeFail);
    if (hit) return (uint32_t)__shfl((int)q, (int)__builtin_ctzll(hit));
  }
  return kLikeFail;
}
// Does the value p[0, len) match?  No backtracking: the first part at the start and the last part at the end where the pattern
// anchors them, the parts between leftmost-first, each behind the one before and in front of an anchored last part.
template <bool WAVE, bool LIT>
__device__ __forceinline__ bool like_match(const uint8_t* p, uint32_t len, const LikePat& P, uint32_t lane) {
  if (len < P.n_elems) return false;
  uint32_t pos = 0, end = len, lo = 0, hi = P.n_parts;
  if (P.flags & LIKE_ANCHOR_START) {
    pos = like_fwd<LIT>(p, 0, len, P, P.parts[0], P.parts[1]);
    if (pos == kLikeFail) return false;
    lo = 1;
    if (hi == 1 && (P.flags & LIKE_ANCHOR_END)) return pos == len;
  }
  if ((P.flags & LIKE_ANCHOR_END) && hi > lo) {
    hi--;
    end = like_bwd<LIT>(p, pos, len, P, P.parts[2 * hi], P.parts[2 * hi + 1]);
    if (end == kLikeFail) return false;
  }
  for (uint32_t k = lo; k < hi; k++) {
    pos = like_find<WAVE, LIT>(p, pos, end, P, P.parts[2 * k], P.parts[2 * k + 1], lane);
    if (pos == kLikeFail) return false;
  }
  return true;
}

// The LIKE leaves' matcher, in front of filter_eval_kernel on its stream.  blockIdx.y = a LIKE leaf with a plane: instruction
// leaves[blockIdx.y] of the program, which names its plane (FilterInsn::i); a wavefront trip is one 64-bit word of the plane, laid
// out like `keep`: bit = the row's value matches (null rows and rows past n_in: 0).  The compiled pattern is staged in LDS once per
// workgroup.  Values of up to kFilterShortString bytes are matched by their own lane, longer ones one after the other by the whole
// wavefront.  Every load of a value byte is bounded by the value's length.
extern "C" __global__ void __launch_bounds__(256)
filter_like_kernel(const FilterInsn* prog, uint32_t n_insn, const uint32_t* leaves, const uint8_t* lits, const FilterCol* cols, const SelBatch* segs,
                   const unsigned long long* seg_first, uint32_t n_segs, uint64_t n_in, uint32_t B, uint32_t W, unsigned long long* planes, uint32_t n_planes) {
  __shared__ uint32_t pat_s[kLikeBlobMax / 4];
  FilterInsn in;
  if (!filter_leaf(prog, n_insn, leaves, FOP_LIKE, n_planes, &in) || in.cmp == LIKE_ALL) return;
  const uint32_t blob = in.lit_len < kLikeBlobMax ? in.lit_len : kLikeBlobMax;
  for (uint32_t x = threadIdx.x; x < blob; x += 256) reinterpret_cast<uint8_t*>(pat_s)[x] = lits[in.lit_off + x];
  __syncthreads();
  LikePat P;
  P.shape = pat_s[0];
  P.flags = pat_s[1];
  P.n_parts = pat_s[2] < kLikeMaxParts ? pat_s[2] : kLikeMaxParts;
  P.n_elems = pat_s[3] < kLikeMaxBytes ? pat_s[3] : kLikeMaxBytes;
  P.parts = pat_s + kLikeHeaderWords;
  P.bytes = reinterpret_cast<const uint8_t*>(pat_s + kLikeHeaderWords + 2 * P.n_parts);
  P.ones = P.bytes + P.n_elems;
  const bool lit = P.shape != LIKE_GENERAL;  // one part of literal bytes: the prefix, suffix and contains shapes skip the `_` tests
  const FilterCol c = cols[in.col];
  const uint32_t lane = threadIdx.x & 63;
  const FilterWords ws = filter_words(n_in);
  unsigned long long* plane = planes + (uint64_t)in.i * ws.n;
  for (uint64_t w = ws.first; w < ws.n; w += ws.stride) {
    const FilterRow r = filter_row(segs, seg_first, n_segs, n_in, B, w * 64 + lane);
    const bool valid = r.live && filter_valid(c, r.u, r.l, W);
    FilterStr v = {c.chars, 0};
    if (valid) v = filter_value_str(c, r.u, r.l, B);
    const bool is_long = valid && v.len > kFilterShortString;
    bool m = false;
    if (valid && !is_long) m = lit ? like_match<false, true>(v.p, v.len, P, lane) : like_match<false, false>(v.p, v.len, P, lane);
    unsigned long long M = __ballot(m);
    for (unsigned long long todo = __ballot(is_long); todo; todo &= todo - 1) {
      const int src = __builtin_ctzll(todo);
      const uint8_t* p = c.chars + __shfl((long long)(v.p - c.chars), src);
      const uint32_t n = (uint32_t)__shfl((int)v.len, src);
      if (lit ? like_match<true, true>(p, n, P, lane) : like_match<true, false>(p, n, P, lane)) M |= 1ull << src;
    }
    if (lane == 0) plane[w] = M;
  }
}

// ---- IN: the hash set of filter_program.h ----
// (InTable, in_table and in_probe_i64: filter_program.h, where the host can call them too)
__device__ __forceinline__ bool in_probe_dec128(const InTable& t, unsigned long long lo, unsigned long long hi) {
  const uint32_t mask = t.n_slots - 1;
  uint32_t s = in_hash_dec128(lo, hi) & mask;
  for (uint32_t step = 0; step < t.n_slots; step++, s = (s + 1) & mask) {
    if (!((t.occ[s >> 6] >> (s & 63)) & 1)) return false;
    const unsigned long long* k = reinterpret_cast<const unsigned long long*>(t.slots) + 2 * (uint64_t)s;
    if (k[0] == lo && k[1] == hi) return true;
  }
  return false;
}
// p[0, len): every byte load of the value is bounded by its length, every one of a key by the table's bytes
__device__ __forceinline__ bool in_probe_string(const InTable& t, const uint8_t* p, uint32_t len) {
  const uint32_t mask = t.n_slots - 1, h = in_hash_bytes(p, len);
  uint32_t s = h & mask;
  for (uint32_t step = 0; step < t.n_slots; step++, s = (s + 1) & mask) {
    if (!((t.occ[s >> 6] >> (s & 63)) & 1)) return false;
    const uint32_t* k = reinterpret_cast<const uint32_t*>(t.slots) + 4 * (uint64_t)s;
    if (k[0] != h || k[1] != len) continue;
    const uint32_t off = k[2];
    if (off > t.bytes || len > t.bytes - off) continue;
    const uint8_t* q = t.base + off;
    uint32_t x = 0;
    while (x < len && p[x] == q[x]) x++;
    if (x == len) return true;
  }
  return false;
}

// One plane of an IN leaf, probed in the table `tab` (LDS or global memory: the caller's two instantiations)
__device__ __forceinline__ void filter_in_plane(const uint8_t* tab, uint32_t tab_bytes, const FilterCol& c, const SelBatch* segs, const unsigned long long* seg_first,
                                                uint32_t n_segs, uint64_t n_in, uint32_t B, uint32_t W, unsigned long long* plane) {
  const InTable t = in_table(tab, tab_bytes);
  // (the key kind the table was built for must be the one the column is decoded to: the host has checked it; a table that does
  // not fit its column matches nothing)
  const bool fits = t.n_slots && (c.kind == FKIND_STRING ? t.kind == IN_KEY_STRING : c.kind == FKIND_DEC128 ? t.kind == IN_KEY_DEC128
                                                                                    : (c.kind == FKIND_INT || c.kind == FKIND_FLOAT) && t.kind == IN_KEY_I64);
  const uint32_t lane = threadIdx.x & 63;
  const FilterWords ws = filter_words(n_in);
  for (uint64_t w = ws.first; w < ws.n; w += ws.stride) {
    const FilterRow r = filter_row(segs, seg_first, n_segs, n_in, B, w * 64 + lane);
    bool m = false;
    if (fits && r.live && filter_valid(c, r.u, r.l, W)) {
      if (c.kind == FKIND_INT) {
        m = in_probe_i64(t, (unsigned long long)filter_load_i64(c, r.row));
      } else if (c.kind == FKIND_FLOAT) {
        const double v = filter_load_f64(c, r.row);
        m = v == v && in_probe_i64(t, in_float_key(v));  // (a NaN row equals no key)
      } else if (c.kind == FKIND_DEC128) {
        unsigned long long lo, hi;
        filter_load_dec128(c, r.row, &lo, &hi);
        m = in_probe_dec128(t, lo, hi);
      } else {
        const FilterSpan s = filter_str_span(c, r.u, r.l, B);
        // (a length no key has: a non-match from the offsets alone, no byte is loaded)
        if (s.len >= t.min_len && s.len <= t.max_len) m = in_probe_string(t, filter_value_str(c, r.u, s).p, s.len);
      }
    }
    const unsigned long long M = __ballot(m);
    if (lane == 0) plane[w] = M;
  }
}

// The IN leaves' set membership, in front of filter_eval_kernel on its stream.  blockIdx.y = an IN leaf with a table: instruction
// leaves[blockIdx.y] of the program, which names its plane (the IN and the LIKE leaves of a program number their planes together);
// a wavefront trip is one 64-bit word of the plane, laid out like `keep`: bit = the row is valid and its key is in the set (null
// rows and rows past n_in: 0).  A table of up to kInLdsBytes is staged in LDS once per workgroup, a larger one is probed where it
// lies: 65536 int64 keys are 1 MiB of slots, which an XCD's L2 holds.  One lane per value, strings included.
extern "C" __global__ void __launch_bounds__(256)
filter_in_kernel(const FilterInsn* prog, uint32_t n_insn, const uint32_t* leaves, const uint8_t* lits, const FilterCol* cols, const SelBatch* segs,
                 const unsigned long long* seg_first, uint32_t n_segs, uint64_t n_in, uint32_t B, uint32_t W, unsigned long long* planes, uint32_t n_planes) {
  __shared__ unsigned long long tab_s[kInLdsBytes / 8];
  FilterInsn in;
  if (!filter_leaf(prog, n_insn, leaves, FOP_IN, n_planes, &in, FOP_IN_SET) || (in.cmp & IN_NO_TABLE)) return;
  const FilterCol c = cols[in.col];
  unsigned long long* plane = planes + (uint64_t)in.i * ((n_in + 63) / 64);
  // (lit_off and lit_len are multiples of 8 and the pool starts 256-byte aligned: whole 8-byte words.  A key set's sealed table
  // lies in an allocation of its own, 256-byte aligned: lit_off is its address, as the host compiled it from a live, sealed set)
  const unsigned long long* g = in.op == FOP_IN_SET ? reinterpret_cast<const unsigned long long*>((uintptr_t)in.lit_off)
                                                    : reinterpret_cast<const unsigned long long*>(lits + in.lit_off);
  const uint32_t bytes = in.lit_len & ~7u;
  if (bytes >= kInHeaderBytes && bytes <= kInLdsBytes) {
    for (uint32_t x = threadIdx.x; x < bytes / 8; x += 256) tab_s[x] = g[x];
    __syncthreads();
    filter_in_plane(reinterpret_cast<const uint8_t*>(tab_s), bytes, c, segs, seg_first, n_segs, n_in, B, W, plane);
  } else {
    filter_in_plane(reinterpret_cast<const uint8_t*>(g), bytes < kInHeaderBytes ? 0 : bytes, c, segs, seg_first, n_segs, n_in, B, W, plane);
  }
}

// ---- expression leaves: both sides by the expression aggregates' evaluator, then the comparison of filter_expr_eval.h ----
// What agg_expr_eval_* reads of a row
struct FilterExprRow {
  const FilterCol* cols;
  FilterRow r;
  uint32_t W;
  __device__ __forceinline__ bool valid(uint32_t col) const { return filter_valid(cols[col], r.u, r.l, W); }
  __device__ __forceinline__ agg_i128 load_int(uint32_t col) const { return (agg_i128)filter_load_i64(cols[col], r.row); }
  __device__ __forceinline__ agg_i128 load_dec(uint32_t col) const {
    unsigned long long lo, hi;
    filter_load_dec128(cols[col], r.row, &lo, &hi);
    return agg_i128_of(lo, hi);
  }
  __device__ __forceinline__ double load_f64(uint32_t col) const { return filter_load_f64(cols[col], r.row); }
};

// The expression leaves' two sides, in front of filter_eval_kernel on its stream.  blockIdx.y = an expression leaf: instruction
// leaves[blockIdx.y] of the program, which names its T plane (FilterInsn::i; i + 1: its F plane, numbered with the LIKE and IN
// planes); a wavefront trip is one 64-bit word of each, laid out like `keep`: T bit = the comparison is TRUE for the row, F bit =
// it is FALSE; neither (UNKNOWN): a column of either side is NULL, or an operation inside a side left 128 bits -- the latter rows
// are counted, one add per block into *overflow.  Rows past n_in: neither.  Both op tables lie in the literal pool and are read
// at wave-uniform addresses; the operand slots are named values (AggSlots): no indexed private array, no scratch.
// (The body of two kernels: DIV = false is filter_expr_kernel; DIV = true, the interpreter with the divide, is filter_expr_div_kernel,
// launched in its place when a leaf of the call holds a division.
// Resource usage (gfx950): filter_expr_kernel 71 VGPRs, 106 SGPRs, 7 waves / SIMD; filter_expr_div_kernel 78 VGPRs, 106 SGPRs, 6 waves /
// SIMD -- the occupancy step the divide costs, paid only by a call that divides; both 16 bytes of LDS, no scratch.)
template <bool DIV, bool COND = false, bool CONV = false>
__device__ __forceinline__ void filter_expr_body(const FilterInsn* prog, uint32_t n_insn, const uint32_t* leaves, const uint8_t* lits, const FilterCol* cols, const SelBatch* segs,
                                                 const unsigned long long* seg_first, uint32_t n_segs, uint64_t n_in, uint32_t B, uint32_t W, unsigned long long* planes,
                                                 uint32_t n_planes, unsigned long long* overflow, uint32_t* over_s) {
  FilterInsn in;
  FilterExprBlob e;
  if (!filter_leaf(prog, n_insn, leaves, FOP_CMP_EXPR, n_planes, &in) || (unsigned long long)in.i + 1 >= n_planes || in.cmp > 5) return;
  if (!filter_expr_blob(lits + in.lit_off, in.lit_len, &e)) return;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const FilterWords ws = filter_words(n_in);
  unsigned long long* plane_t = planes + (uint64_t)in.i * ws.n;
  unsigned long long* plane_f = plane_t + ws.n;
  uint32_t n_over = 0;  // (wave-uniform: popcounts of ballots)
  for (uint64_t w = ws.first; w < ws.n; w += ws.stride) {
    const FilterExprRow row = {cols, filter_row(segs, seg_first, n_segs, n_in, B, w * 64 + lane), W};
    bool t = false, known = false, over = false;
    if (row.r.live) {
      int sl, sr;
      if (e.cls == FXC_FLOAT) {
        double a = 0.0, b = 0.0;
        sl = agg_expr_eval_f64_as<DIV, COND, CONV>(e.lhs, e.n_lhs, row, &a);
        sr = agg_expr_eval_f64_as<DIV, COND, CONV>(e.rhs, e.n_rhs, row, &b);
        known = sl == AGG_ROW_VALUE && sr == AGG_ROW_VALUE;
        if constexpr (CONV) over = sl != AGG_ROW_NULL && sr != AGG_ROW_NULL && !known;  // (a conversion inside a side of doubles can overflow)
        t = known && filter_expr_compare_f64(in.cmp, a, b);
      } else {
        agg_i128 a = 0, b = 0;
        sl = agg_expr_eval_i128_as<DIV, COND, CONV>(e.lhs, e.n_lhs, row, &a);
        sr = agg_expr_eval_i128_as<DIV, COND, CONV>(e.rhs, e.n_rhs, row, &b);
        known = sl == AGG_ROW_VALUE && sr == AGG_ROW_VALUE;
        over = sl != AGG_ROW_NULL && sr != AGG_ROW_NULL && !known;  // (a NULL column comes first: the row is not counted)
        t = known && filter_expr_compare_i128(in.cmp, a, b, e.d, e.p10);
      }
    }
    const unsigned long long T = __ballot(t), F = __ballot(known && !t);
    n_over += (uint32_t)__builtin_popcountll(__ballot(over));
    if (lane == 0) {
      plane_t[w] = T;
      plane_f[w] = F;
    }
  }
  if (lane == 0) over_s[wave] = n_over;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long n = (unsigned long long)over_s[0] + over_s[1] + over_s[2] + over_s[3];
    if (n) atomicAdd(overflow, n);
  }
}
extern "C" __global__ void __launch_bounds__(256)
filter_expr_kernel(const FilterInsn* prog, uint32_t n_insn, const uint32_t* leaves, const uint8_t* lits, const FilterCol* cols, const SelBatch* segs,
                   const unsigned long long* seg_first, uint32_t n_segs, uint64_t n_in, uint32_t B, uint32_t W, unsigned long long* planes, uint32_t n_planes,
                   unsigned long long* overflow) {
  __shared__ uint32_t over_s[4];
  filter_expr_body<false>(prog, n_insn, leaves, lits, cols, segs, seg_first, n_segs, n_in, B, W, planes, n_planes, overflow, over_s);
}
extern "C" __global__ void __launch_bounds__(256)
filter_expr_div_kernel(const FilterInsn* prog, uint32_t n_insn, const uint32_t* leaves, const uint8_t* lits, const FilterCol* cols, const SelBatch* segs,
                       const unsigned long long* seg_first, uint32_t n_segs, uint64_t n_in, uint32_t B, uint32_t W, unsigned long long* planes, uint32_t n_planes,
                       unsigned long long* overflow) {
  __shared__ uint32_t over_s[4];
  filter_expr_body<true>(prog, n_insn, leaves, lits, cols, segs, seg_first, n_segs, n_in, B, W, planes, n_planes, overflow, over_s);
}
// (the interpreter with the divide and the conditionals: launched when a leaf of the call holds a conditional op)
extern "C" __global__ void __launch_bounds__(256)
filter_expr_cond_kernel(const FilterInsn* prog, uint32_t n_insn, const uint32_t* leaves, const uint8_t* lits, const FilterCol* cols, const SelBatch* segs,
                        const unsigned long long* seg_first, uint32_t n_segs, uint64_t n_in, uint32_t B, uint32_t W, unsigned long long* planes, uint32_t n_planes,
                        unsigned long long* overflow) {
  __shared__ uint32_t over_s[4];
  filter_expr_body<true, true>(prog, n_insn, leaves, lits, cols, segs, seg_first, n_segs, n_in, B, W, planes, n_planes, overflow, over_s);
}
// (the mixed interpreter: launched when a leaf of the call holds a conversion)
extern "C" __global__ void __launch_bounds__(256)
filter_expr_conv_kernel(const FilterInsn* prog, uint32_t n_insn, const uint32_t* leaves, const uint8_t* lits, const FilterCol* cols, const SelBatch* segs,
                        const unsigned long long* seg_first, uint32_t n_segs, uint64_t n_in, uint32_t B, uint32_t W, unsigned long long* planes, uint32_t n_planes,
                        unsigned long long* overflow) {
  __shared__ uint32_t over_s[4];
  filter_expr_body<true, true, true>(prog, n_insn, leaves, lits, cols, segs, seg_first, n_segs, n_in, B, W, planes, n_planes, overflow, over_s);
}

// One 64-row word of a predicate: the program prog[0, n_insn) over the trip's rows -- lane l holds input row w * 64 + l as `r`,
// live_m = the ballot of r.live --, evaluated as the head comment says: a leaf yields two ballot words, inner nodes combine words on
// the wavefront's own stack (stk_t / stk_f: kFilterStack words each, in LDS).  Returns the rows where the root is TRUE, live rows
// only.  planes: the LIKE / IN leaves' match bits, n_words words a plane.  What filter_eval_kernel runs for the row filter and
// agg_cond_eval_kernel (agg_kernels.hip) for an aggregate's condition.
__device__ __forceinline__ unsigned long long filter_eval_word(const FilterInsn* prog, uint32_t n_insn, const uint8_t* lits, const FilterCol* cols, const FilterRow& r,
                                                               unsigned long long live_m, uint32_t B, uint32_t W, const unsigned long long* planes, uint64_t n_words,
                                                               uint64_t w, unsigned long long* stk_t, unsigned long long* stk_f) {
  uint32_t sp = 0;
  for (uint32_t k = 0; k < n_insn; k++) {
    const FilterInsn in = prog[k];
    unsigned long long T = 0, F = 0;
    if (in.op <= FOP_IS_NOT_NULL) {
      const FilterCol c = cols[in.col];
      const bool valid = r.live && filter_valid(c, r.u, r.l, W);
      bool t = false, f = false;
      if (in.op == FOP_IS_NULL) {
        t = r.live && !valid;
        f = valid;
      } else if (in.op == FOP_IS_NOT_NULL) {
        t = valid;
        f = r.live && !valid;
      } else if (valid) {
        bool lt = false, eq = false, gt = false;
        if (in.op == FOP_CMP_INT || in.op == FOP_CMP_BOOL) {
          const long long v = in.op == FOP_CMP_INT ? filter_load_i64(c, r.row) : (long long)filter_load_bit(c, r.u, r.l, W);
          lt = v < in.i;
          eq = v == in.i;
          gt = v > in.i;
        } else if (in.op == FOP_CMP_FLOAT) {
          const double v = filter_load_f64(c, r.row);
          lt = v < in.f;
          eq = v == in.f;
          gt = v > in.f;
        } else if (in.op == FOP_CMP_DEC128) {  // the high words as signed, the low words as unsigned
          unsigned long long vl, hi;
          filter_load_dec128(c, r.row, &vl, &hi);
          const long long vh = (long long)hi;
          eq = vh == in.i && vl == in.lo;
          lt = vh < in.i || (vh == in.i && vl < in.lo);
          gt = !lt && !eq;
        } else {  // FOP_CMP_STRING
          const FilterStr v = filter_value_str(c, r.u, r.l, B);
          const uint8_t* q = lits + in.lit_off;
          const uint32_t m = v.len < in.lit_len ? v.len : in.lit_len;
          uint32_t x = 0;
          while (x < m && v.p[x] == q[x]) x++;
          if (x < m) {
            lt = v.p[x] < q[x];
            gt = !lt;
          } else {
            lt = v.len < in.lit_len;
            eq = v.len == in.lit_len;
            gt = v.len > in.lit_len;
          }
        }
        switch (in.cmp) {
          case 0: t = eq; break;         // EQ
          case 1: t = !eq; break;        // NE (true with a NaN on either side)
          case 2: t = lt; break;         // LT
          case 3: t = lt || eq; break;   // LE
          case 4: t = gt; break;         // GT
          default: t = gt || eq; break;  // GE
        }
        f = !t;
      }
      T = __ballot(t);
      F = __ballot(f);
    } else if (in.op == FOP_LIKE) {
      // the trip's match bits are there already (filter_like_kernel); only `%`: every valid row, and no plane to load
      const unsigned long long valid_m = __ballot(r.live && filter_valid(cols[in.col], r.u, r.l, W));
      const unsigned long long match = in.cmp == LIKE_ALL ? ~0ull : planes[(uint64_t)in.i * n_words + w];
      T = match & valid_m;
      F = ~match & valid_m;
    } else if (in.op == FOP_IN || in.op == FOP_IN_SET) {
      // the trip's membership bits are there already (filter_in_kernel); a Boolean column and a list no key of which can equal a
      // row have no plane.  With a NULL literal in the list a row that matches no key is UNKNOWN, not FALSE.
      const FilterCol c = cols[in.col];
      const bool valid = r.live && filter_valid(c, r.u, r.l, W);
      const unsigned long long valid_m = __ballot(valid);
      unsigned long long match = 0;
      if (!(in.cmp & IN_NO_TABLE)) match = planes[(uint64_t)in.i * n_words + w];
      else if (in.cmp & (IN_BOOL_FALSE | IN_BOOL_TRUE)) {
        const unsigned long long bits = __ballot(valid && filter_load_bit(c, r.u, r.l, W));
        match = (in.cmp & IN_BOOL_TRUE ? bits : 0ull) | (in.cmp & IN_BOOL_FALSE ? ~bits : 0ull);
      }
      T = match & valid_m;
      F = in.cmp & IN_HAS_NULL ? 0ull : ~match & valid_m;
    } else if (in.op == FOP_CMP_EXPR) {
      // both answers are there already (filter_expr_kernel): the T plane and the F plane behind it; neither bit: UNKNOWN
      T = planes[(uint64_t)in.i * n_words + w] & live_m;
      F = planes[((uint64_t)in.i + 1) * n_words + w] & live_m;
    } else if (in.op == FOP_TRUE) {
      T = live_m;
    } else if (in.op == FOP_FALSE) {
      F = live_m;
    } else if (in.op == FOP_NOT) {
      sp--;
      T = stk_f[sp];
      F = stk_t[sp];
    } else if (in.op == FOP_AND || in.op == FOP_OR) {
      sp -= 2;
      const unsigned long long t1 = stk_t[sp], f1 = stk_f[sp], t2 = stk_t[sp + 1], f2 = stk_f[sp + 1];
      if (in.op == FOP_AND) {
        T = t1 & t2;
        F = f1 | f2;
      } else {
        T = t1 | t2;
        F = f1 & f2;
      }
    }  // (FOP_UNKNOWN: neither)
    // (every lane holds the same words and writes them to the same slot: the wavefront's stack needs no barrier)
    stk_t[sp] = T;
    stk_f[sp] = F;
    sp++;
  }
  return (sp ? stk_t[0] : 0ull) & live_m;
}

extern "C" __global__ void __launch_bounds__(256)
filter_eval_kernel(const FilterInsn* prog, uint32_t n_insn, const uint8_t* lits, const FilterCol* cols, const SelBatch* segs,
                   const unsigned long long* seg_first, uint32_t n_segs, uint64_t n_in, uint32_t B, uint32_t W, unsigned long long* keep,
                   uint32_t* cnt, const unsigned long long* planes) {
  __shared__ unsigned long long stk_t[4][kFilterStack], stk_f[4][kFilterStack];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const FilterWords ws = filter_words(n_in);
  for (uint64_t w = ws.first; w < ws.n; w += ws.stride) {
    const FilterRow r = filter_row(segs, seg_first, n_segs, n_in, B, w * 64 + lane);
    const unsigned long long root = filter_eval_word(prog, n_insn, lits, cols, r, __ballot(r.live), B, W, planes, ws.n, w, stk_t[wave], stk_f[wave]);
    if (lane == 0) {
      keep[w] = root;
      cnt[w] = (uint32_t)__builtin_popcountll(root);
    }
  }
}

// every kept input row -> src_rows[its output row] = its row of the stripe
extern "C" __global__ void __launch_bounds__(256)
filter_place_kernel(const unsigned long long* keep, const unsigned long long* woff, const SelBatch* segs, const unsigned long long* seg_first,
                    uint32_t n_segs, uint64_t n_in, uint32_t* src_rows) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_in) return;
  const unsigned long long m = keep[j >> 6];
  const uint32_t lane = (uint32_t)(j & 63);
  if (!((m >> lane) & 1)) return;
  const uint64_t o = woff[j >> 6] + (uint64_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
  src_rows[o] = (uint32_t)filter_src_row(segs, seg_first, n_segs, j);
}

// blockIdx.x = output batch (of at most nb_max; those past the kept rows leave at once), blockIdx.y = column.
// nulls / char_total: [column][nb_max], zeroed by the host
extern "C" __global__ void __launch_bounds__(256)
filter_count_kernel(const FilterCol* cols, const uint32_t* src_rows, const unsigned long long* total, uint32_t B, uint32_t W, uint32_t nb_max,
                    unsigned long long* nulls, unsigned long long* char_total) {
  const FilterCol c = cols[blockIdx.y];
  const uint64_t kept = *total, first = (uint64_t)blockIdx.x * B;
  if (first >= kept || (!c.validity && c.kind != FKIND_STRING)) return;
  const uint32_t len = (uint32_t)(kept - first < B ? kept - first : B);
  unsigned long long n_null = 0, n_bytes = 0;
  for (uint32_t i = threadIdx.x; i < len; i += 256) {
    const FilterRow r = filter_row_of(src_rows[first + i], B);
    if (!filter_valid(c, r.u, r.l, W)) n_null++;
    if (c.kind == FKIND_STRING) n_bytes += filter_str_len(c, r.u, r.l, B);
  }
  for (int o = 32; o; o >>= 1) {
    n_null += (unsigned long long)__shfl_xor((long long)n_null, o);
    n_bytes += (unsigned long long)__shfl_xor((long long)n_bytes, o);
  }
  if ((threadIdx.x & 63) == 0) {
    const uint64_t at = (uint64_t)blockIdx.y * nb_max + blockIdx.x;
    if (n_null) atomicAdd(&nulls[at], n_null);
    if (n_bytes) atomicAdd(&char_total[at], n_bytes);
  }
}

// `len` values of type T from rows[] of src to contiguous out: 16-byte stores (16 / sizeof(T) values a lane) when out is 16-byte
// aligned, the tail and unaligned batches value by value
template <typename T>
__device__ __forceinline__ void filter_gather_fixed(const uint8_t* src_, uint8_t* out_, const uint32_t* rows, uint32_t len) {
  const T* src = reinterpret_cast<const T*>(src_);
  T* out = reinterpret_cast<T*>(out_);
  constexpr uint32_t R = 16 / sizeof(T);
  uint32_t done = 0;
  if ((reinterpret_cast<uintptr_t>(out_) & 15) == 0) {
    const uint32_t groups = len / R;
    for (uint32_t g = threadIdx.x; g < groups; g += 256) {
      union {
        T v[R];
        uint4 q;
      } x;
#pragma unroll
      for (uint32_t r = 0; r < R; r++) x.v[r] = src[rows[g * R + r]];
      reinterpret_cast<uint4*>(out_)[g] = x.q;
    }
    done = groups * R;
  }
  for (uint32_t i = done + threadIdx.x; i < len; i += 256) out[i] = src[rows[i]];
}
struct FilterV16 {
  unsigned long long lo, hi;
};

// blockIdx.x = output batch (exactly those of the kept rows), blockIdx.y = column
extern "C" __global__ void __launch_bounds__(256)
filter_gather_kernel(const FilterGatherJob* jobs, const uint32_t* src_rows, uint64_t kept, uint32_t B, uint32_t W) {
  __shared__ unsigned long long wsum[4];
  __shared__ unsigned long long carry_s;
  const FilterGatherJob j = jobs[blockIdx.y];
  const FilterCol& c = j.src;
  const uint64_t ob = blockIdx.x, first = ob * B;
  if (first >= kept) return;
  const uint32_t len = (uint32_t)(kept - first < B ? kept - first : B);
  const uint32_t* rows = src_rows + first;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // ---- validity and Boolean value bits, by ballot ----
  if (j.out_validity || c.kind == FKIND_BOOL) {
    for (uint32_t i0 = 0; i0 < len; i0 += 256) {
      const uint32_t i = i0 + threadIdx.x;
      const FilterRow r = filter_row_of(i < len ? rows[i] : 0, B, i < len);
      const unsigned long long lm = __ballot(r.live);
      if (j.out_validity) {
        const unsigned long long vm = __ballot(r.live && filter_valid(c, r.u, r.l, W));
        if (lane == 0 && lm) j.out_validity[ob * W + (i >> 6)] = vm;
      }
      if (c.kind == FKIND_BOOL) {
        const unsigned long long bm = __ballot(r.live && filter_load_bit(c, r.u, r.l, W));
        if (lane == 0 && lm) reinterpret_cast<unsigned long long*>(j.out_values)[ob * W + (i >> 6)] = bm;
      }
    }
  }
  if (c.kind == FKIND_BOOL) return;
  // ---- fixed-width values ----
  if (c.kind != FKIND_STRING) {
    uint8_t* out = j.out_values + first * c.width;
    switch (c.width) {
      case 1: filter_gather_fixed<uint8_t>(c.values, out, rows, len); break;
      case 2: filter_gather_fixed<uint16_t>(c.values, out, rows, len); break;
      case 4: filter_gather_fixed<uint32_t>(c.values, out, rows, len); break;
      case 8: filter_gather_fixed<unsigned long long>(c.values, out, rows, len); break;
      case 16: filter_gather_fixed<FilterV16>(c.values, out, rows, len); break;
      default: break;
    }
    return;
  }
  // ---- strings: lengths -> offsets of the batch (exclusive scan, restarting at 0) ----
  int32_t* ooff = j.out_offsets + ob * (B + 1);
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (uint32_t i0 = 0; i0 < len; i0 += 256) {
    const uint32_t i = i0 + threadIdx.x;
    unsigned long long n = 0;
    if (i < len) {
      const FilterRow r = filter_row_of(rows[i], B);
      n = filter_str_len(c, r.u, r.l, B);
    }
    unsigned long long inc = n;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long y = (unsigned long long)__shfl_up((long long)inc, o);
      if (lane >= (uint32_t)o) inc += y;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned long long before = carry_s;
    for (uint32_t x = 0; x < wave; x++) before += wsum[x];
    if (i < len) ooff[i] = (int32_t)(uint32_t)(before + inc - n);
    __syncthreads();
    if (threadIdx.x == 255) carry_s = before + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) ooff[len] = (int32_t)(uint32_t)carry_s;
  // ---- ... and the bytes: a lane per short value, then a wavefront per long one ----
  uint8_t* dst0 = j.out_chars + j.out_char_base[ob];
  // (both loops read the offsets pair themselves, not through filter_str_span: the length tests and the copy loop's own then
  // compile to one branch per value, which matters to a block that walks a batch's rows one after the other)
  for (uint32_t i = threadIdx.x; i < len; i += 256) {
    const FilterRow r = filter_row_of(rows[i], B);
    const int32_t* o = filter_str_offsets(c, r.u, r.l, B);
    const uint32_t a = (uint32_t)o[0], n = (uint32_t)o[1] - a;
    if (n == 0 || n > kFilterShortString) continue;
    const FilterStr v = filter_value_str(c, r.u, FilterSpan{a, n});
    uint8_t* d = dst0 + (uint32_t)ooff[i];
    for (uint32_t x = 0; x < v.len; x++) d[x] = v.p[x];
  }
  for (uint32_t i = wave; i < len; i += 4) {
    const FilterRow r = filter_row_of(rows[i], B);
    const int32_t* o = filter_str_offsets(c, r.u, r.l, B);
    const uint32_t a = (uint32_t)o[0], n = (uint32_t)o[1] - a;
    if (n <= kFilterShortString) continue;
    const FilterStr v = filter_value_str(c, r.u, FilterSpan{a, n});
    uint8_t* d = dst0 + (uint32_t)ooff[i];
    for (uint32_t x = lane; x < n; x += 64) d[x] = v.p[x];
  }
}
