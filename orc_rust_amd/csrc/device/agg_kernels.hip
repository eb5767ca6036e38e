// agg_kernels.hip -- COUNT, SUM, MIN, MAX and the one product SUM(a * b) over the KEPT rows of a decoded stripe, reduced where the
// rows lie: nothing is scanned, placed, gathered or copied back but one record per aggregate.
//
// The reference has no aggregation; the semantics are those of include/orcgpu.h (orcgpu_result_aggregate).  The kept rows are
// the bits of the keep mask filter_eval_kernel leaves (filter_kernels.hip), or -- without a filter -- every input row.
//
//   agg_partial_kernel   grid (agg_blocks(n_in), instructions).  A wavefront takes one 64-row word of the keep mask per trip and
//                        passes over the words that are 0; a lane loads its row through the row-access layer (filter_access.h) and
//                        adds it to an accumulator of its own.  Behind the last trip the wavefront folds its 64 accumulators with
//                        shuffles in a fixed tree, the block its four wavefronts through LDS in wavefront order: ONE record per
//                        (block, instruction).
//   agg_final_kernel     one block per instruction: thread t folds records t, t + 256, ... in index order, then the same tree.
//   agg_expr_partial_kernel  agg_partial_kernel for the instructions that sum an arithmetic expression (AK_EXPR_*): the same grid,
//                        the same records, the same folds; a lane runs the instruction's program (agg_expr_eval.h) on its row.
//                        A kernel of its own, launched only when the list holds such an instruction, so that the interpreter's
//                        registers are not the plain kinds'; each of the two kernels leaves the other's rows of grid.y at once.
//                        The two are one body, agg_partial_body<EXPR>; the rows they walk arrive as one argument (KeptRows).
//
//   agg_cond_eval_kernel     in front of all of them when an aggregate carries a condition (AggInsn::cond, agg(x) FILTER (WHERE ...)):
//                        one mask plane per distinct condition, laid out like the keep mask, = the rows that are kept AND for which
//                        the condition is TRUE, evaluated by the row filter's own per-word evaluation (filter_eval_word).  A
//                        conditioned instruction reduces its plane where the others reduce the keep mask.
//
// Integer and Decimal sums travel as three 64-bit words with explicit carries -- wide enough for every partial sum, so the
// order of summation cannot show.  Float sums take whatever the fixed shape gives: the grid is a function of the input row
// count alone (agg_program.h), there is no atomic anywhere, and so the same call gives the same bits.
#pragma once
#include <stdint.h>

#include "agg_expr_eval.h"
#include "agg_program.h"
#include "filter_access.h"
#include "filter_kernels.hip"
#include "filter_program.h"

struct AggAcc {
  unsigned long long w0, w1, w2;
  double f;
  unsigned long long count;
  uint32_t flags;
};

// a += b over signed 192-bit integers in two's complement
__device__ __forceinline__ void agg_add192(AggAcc& a, unsigned long long b0, unsigned long long b1, unsigned long long b2) {
  const unsigned long long r0 = a.w0 + b0;
  const unsigned long long c0 = r0 < b0;
  const unsigned long long t1 = a.w1 + b1;
  const unsigned long long c1 = t1 < b1;
  const unsigned long long r1 = t1 + c0;
  const unsigned long long c2 = r1 < c0;
  a.w0 = r0;
  a.w1 = r1;
  a.w2 = a.w2 + b2 + c1 + c2;
}
__device__ __forceinline__ void agg_add_i64(AggAcc& a, long long v) {
  const unsigned long long s = (unsigned long long)(v >> 63);
  agg_add192(a, (unsigned long long)v, s, s);
}
__device__ __forceinline__ void agg_add_i128(AggAcc& a, unsigned long long lo, unsigned long long hi) {
  agg_add192(a, lo, hi, (unsigned long long)((long long)hi >> 63));
}
__device__ __forceinline__ bool agg_less_i128(unsigned long long alo, unsigned long long ahi, unsigned long long blo, unsigned long long bhi) {
  return (long long)ahi < (long long)bhi || (ahi == bhi && alo < blo);
}

// a <- a (+) b: what two accumulators of one instruction fold to.  `a` stands in front of `b` in the fixed order.
__device__ __forceinline__ void agg_fold(uint32_t kind, bool is_max, AggAcc& a, const AggAcc& b) {
  a.flags |= b.flags;
  if (agg_is_float_sum(kind)) {
    a.f += b.f;
  } else if (agg_is_wide_sum(kind)) {
    agg_add192(a, b.w0, b.w1, b.w2);
  } else if (b.count) {
    bool take = !a.count;
    if (!take) {
      if (kind == AK_MINMAX_INT) take = is_max ? (long long)b.w0 > (long long)a.w0 : (long long)b.w0 < (long long)a.w0;
      else if (kind == AK_MINMAX_DEC) take = is_max ? agg_less_i128(a.w0, a.w1, b.w0, b.w1) : agg_less_i128(b.w0, b.w1, a.w0, a.w1);
      else take = is_max ? b.f > a.f : b.f < a.f;
    }
    if (take) {
      a.w0 = b.w0;
      a.w1 = b.w1;
      a.f = b.f;
    }
  }
  a.count += b.count;
}

__device__ __forceinline__ unsigned long long agg_shfl_down(unsigned long long v, int o) { return (unsigned long long)__shfl_down((long long)v, o); }
// The wavefront's 64 accumulators -> lane 0's, in the tree ((0 + 32) + (16 + 48)) + ... of shuffles down by 32, 16, .. 1
__device__ __forceinline__ void agg_wave_fold(uint32_t kind, bool is_max, AggAcc& a) {
  for (int o = 32; o; o >>= 1) {
    AggAcc b;
    b.w0 = agg_shfl_down(a.w0, o);
    b.w1 = agg_shfl_down(a.w1, o);
    b.w2 = agg_shfl_down(a.w2, o);
    b.f = __shfl_down(a.f, o);
    b.count = agg_shfl_down(a.count, o);
    b.flags = (uint32_t)__shfl_down((int)a.flags, o);
    agg_fold(kind, is_max, a, b);
  }
}
// ... and the block's four wavefronts -> thread 0's, through LDS in wavefront order
__device__ __forceinline__ void agg_block_fold(uint32_t kind, bool is_max, AggAcc& a, AggAcc* lds) {
  agg_wave_fold(kind, is_max, a);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0)
    for (uint32_t x = 1; x < 4; x++) agg_fold(kind, is_max, a, lds[x]);
}
__device__ __forceinline__ void agg_store(AggPartial* out, const AggAcc& a) {
  out->w[0] = a.w0;
  out->w[1] = a.w1;
  out->w[2] = a.w2;
  out->f = a.f;
  out->count = a.count;
  out->flags = a.flags;
  out->pad = 0;
}

// One value into a lane's accumulator: MIN / MAX of what is there and (w0, w1 | f)
__device__ __forceinline__ void agg_minmax(uint32_t kind, bool is_max, AggAcc& a, unsigned long long w0, unsigned long long w1, double f) {
  AggAcc b = {w0, w1, 0, f, 1, 0};
  agg_fold(kind, is_max, a, b);
}

// One kept row into an accumulator of instruction `in` (any kind but AK_COUNT_ROWS, which reads no row): what agg_partial_kernel
// and agg_group_partial_kernel (agg_group_kernels.hip) do per lane.  A null value adds nothing.
__device__ __forceinline__ void agg_row(uint32_t kind, bool is_max, const AggInsn& in, const FilterCol& c, const FilterCol& c2, const FilterRow& r, uint32_t W,
                                        AggAcc& a) {
  if (!r.live || !filter_valid(c, r.u, r.l, W)) return;
  switch (kind) {
    case AK_COUNT: a.w0++; break;
    case AK_SUM_INT:
      agg_add_i64(a, filter_load_i64(c, r.row));
      a.count++;
      break;
    case AK_SUM_DEC: {
      unsigned long long lo, hi;
      filter_load_dec128(c, r.row, &lo, &hi);
      agg_add_i128(a, lo, hi);
      a.count++;
      break;
    }
    case AK_SUM_F64:
      a.f += filter_load_f64(c, r.row);
      a.count++;
      break;
    case AK_SP_INT:
    case AK_SP_DEC: {
      if (!filter_valid(c2, r.u, r.l, W)) break;
      long long x, y;
      if (kind == AK_SP_INT) {
        x = filter_load_i64(c, r.row);
        y = filter_load_i64(c2, r.row);
      } else {
        unsigned long long xl, xh, yl, yh;
        filter_load_dec128(c, r.row, &xl, &xh);
        filter_load_dec128(c2, r.row, &yl, &yh);
        if (xh != (unsigned long long)((long long)xl >> 63) || yh != (unsigned long long)((long long)yl >> 63)) {
          a.flags |= AGG_OVERFLOW;  // an operand that does not fit a signed 64-bit word: sticky, the row is left out
          a.count++;
          break;
        }
        x = (long long)xl;
        y = (long long)yl;
      }
      const __int128 p = (__int128)x * (__int128)y;
      agg_add_i128(a, (unsigned long long)p, (unsigned long long)(p >> 64));
      a.count++;
      break;
    }
    case AK_SP_F64:
      if (!filter_valid(c2, r.u, r.l, W)) break;
      a.f += filter_load_f64(c, r.row) * filter_load_f64(c2, r.row);
      a.count++;
      break;
    case AK_MINMAX_INT: {
      const long long v = in.fkind == FKIND_BOOL ? (long long)filter_load_bit(c, r.u, r.l, W) : filter_load_i64(c, r.row);
      agg_minmax(kind, is_max, a, (unsigned long long)v, 0, 0.0);
      break;
    }
    case AK_MINMAX_DEC: {
      unsigned long long lo, hi;
      filter_load_dec128(c, r.row, &lo, &hi);
      agg_minmax(kind, is_max, a, lo, hi, 0.0);
      break;
    }
    default: {  // AK_MINMAX_F64
      const double v = filter_load_f64(c, r.row);
      if (v != v) a.flags |= AGG_SAW_NAN;
      else agg_minmax(kind, is_max, a, 0, 0, v);
      break;
    }
  }
}

// A row as the expression evaluator reads it: the columns through the row-access layer.  `col` comes from the program, which the
// host checked against the column table; it is uniform over the wavefront, so a column's description is read by scalar loads.
struct AggExprRow {
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

#pragma clang fp contract(off)  // (the sum's addition is an operation of its own, never fused with the expression's last multiply)
// One kept row into an accumulator of an AK_EXPR_* instruction whose program is prog[0 .. n): a row with a NULL operand adds
// nothing; a row whose value left 128 bits counts, sets the sticky flag and adds nothing
// (CONV: the mixed interpreter -- conversions, include/orcgpu.h: CONVERSIONS --, in which a row of the FLOAT class can overflow too)
template <bool DIV, bool COND = false, bool CONV = false>
__device__ __forceinline__ void agg_expr_row(uint32_t kind, const AggExprOp* prog, uint32_t n, const FilterCol* cols, const FilterRow& r, uint32_t W, AggAcc& a) {
  if (!r.live) return;
  const AggExprRow row = {cols, r, W};
  if (kind == AK_EXPR_F64) {
    double v;
    const int rc = agg_expr_eval_f64_as<DIV, COND, CONV>(prog, n, row, &v);
    if (rc == AGG_ROW_NULL) return;
    if (CONV && rc == AGG_ROW_OVERFLOW) a.flags |= AGG_OVERFLOW;
    else a.f += v;
  } else {
    agg_i128 v;
    const int rc = agg_expr_eval_i128_as<DIV, COND, CONV>(prog, n, row, &v);
    if (rc == AGG_ROW_NULL) return;
    if (rc == AGG_ROW_OVERFLOW) a.flags |= AGG_OVERFLOW;
    else agg_add_i128(a, (unsigned long long)v, (unsigned long long)((agg_u128)v >> 64));
  }
  a.count++;
}
#pragma clang fp contract(fast)  // (what the rest of the library is built with)

// Word w of the keep mask (w below the word count): without a filter every input row is kept, the last word up to n_in
__device__ __forceinline__ unsigned long long agg_keep_word(const KeptRows& rows, uint64_t w) {
  const uint64_t left = rows.n_in - w * 64;  // (at least 1)
  return rows.keep ? rows.keep[w] : (left >= 64 ? ~0ull : (1ull << left) - 1ull);
}

// The plane of an instruction's condition (cond = k + 1: plane k, which agg_cond_eval_kernel left as "kept, and the condition is
// TRUE"), found once per kernel: null without a condition.  *blocked: a plane past those of the call -- the host refuses such a
// plan before any launch (agg_plan_in_bounds); here no row passes and nothing is loaded.
__device__ __forceinline__ const unsigned long long* agg_cond_plane(const KeptRows& rows, uint32_t cond, bool* blocked) {
  *blocked = cond > rows.n_cond;
  return cond && !*blocked ? rows.cond + (uint64_t)(cond - 1) * ((rows.n_in + 63) / 64) : nullptr;
}
// Does the kept input row j (below n_in) pass?  What the grouped kernels ask per row
__device__ __forceinline__ bool agg_row_passes(const unsigned long long* plane, uint64_t j) { return !plane || ((plane[j >> 6] >> (j & 63)) & 1); }

// The planes of an aggregate list's distinct conditions, in front of the partial kernels on their stream.  grid (blocks over the
// words as filter_eval_kernel's, conditions): blockIdx.y = condition k, whose program is prog[spans[k].first, + spans[k].n) of the
// call's predicate program (the row filter's instructions, then the conditions'; a span that leaves it evaluates to no row).
// out[k][w] = TRUE-word of condition k & keep word: EVERY word of every plane is written on every call, a word whose keep word
// is 0 as 0 without a row being loaded.  The LIKE / IN leaves of the conditions find their match bits in leaf_planes, where
// filter_like_kernel / filter_in_kernel left them.
extern "C" __global__ void __launch_bounds__(256)
agg_cond_eval_kernel(const FilterInsn* prog, uint32_t n_insn, const AggCondSpan* spans, const uint8_t* lits, KeptRows rows, const unsigned long long* leaf_planes,
                     unsigned long long* out) {
  __shared__ unsigned long long stk_t[4][kFilterStack], stk_f[4][kFilterStack];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  AggCondSpan span = spans[blockIdx.y];
  if (span.first > n_insn || span.n > n_insn - span.first) span.n = 0;
  const FilterWords ws = filter_words(rows.n_in);
  unsigned long long* plane = out + (uint64_t)blockIdx.y * ws.n;
  for (uint64_t w = ws.first; w < ws.n; w += ws.stride) {
    const unsigned long long m = agg_keep_word(rows, w);
    unsigned long long pass = 0;
    if (m && span.n) {  // (uniform over the wavefront)
      const FilterRow r = filter_row(rows, w * 64 + lane);
      pass = filter_eval_word(prog + span.first, span.n, lits, rows.cols, r, __ballot(r.live), rows.B, rows.W, leaf_planes, ws.n, w, stk_t[wave], stk_f[wave]) & m;
    }
    if (lane == 0) plane[w] = pass;
  }
}

// partials: [instruction][block].  A lane whose row is not kept loads nothing; a kept row is an input row below n_in, and the
// row-access layer turns it into a row of the stripe: every load lies where the decode wrote.
// (The body of two kernels: EXPR = false is agg_partial_kernel, which takes the plain kinds and leaves the AK_EXPR_* rows of grid.y
// at once -- their col / col2 are no column indexes; EXPR = true is agg_expr_partial_kernel, the other way round.  ops: the op
// table the instructions' programs lie in, EXPR only.  DIV: the interpreter with the divide -- agg_expr_div_partial_kernel, launched
// in place of agg_expr_partial_kernel when a program of the list holds a division.
// Resource usage (gfx950): agg_expr_partial_kernel 73 VGPRs, 106 SGPRs, 6 waves / SIMD; agg_expr_div_partial_kernel 83 VGPRs, 106 SGPRs,
// 5 waves / SIMD -- the occupancy step the divide costs, paid only by a list that divides; both 192 bytes of LDS, no scratch
// (INTEGRATION.md 6o).)
template <bool EXPR, bool DIV = false, bool COND = false, bool CONV = false>
__device__ __forceinline__ void agg_partial_body(const AggInsn* insns, const AggExprOp* ops, const KeptRows& rows, AggPartial* partials, AggAcc* fold_s) {
  const AggInsn in = insns[blockIdx.y];
  if (agg_is_expr(in.kind) != EXPR) return;  // (uniform over the block)
  const uint32_t kind = EXPR ? in.kind : in.kind < AK_N ? in.kind : AK_COUNT_ROWS;
  const bool is_max = !EXPR && in.is_max != 0;
  const FilterCol c = rows.cols[EXPR ? 0 : in.col], c2 = rows.cols[EXPR ? 0 : in.col2];  // (EXPR: unused)
  const uint32_t lane = threadIdx.x & 63;
  const FilterWords ws = filter_words(rows.n_in);
  bool blocked;
  const unsigned long long* const plane = agg_cond_plane(rows, in.cond, &blocked);
  AggAcc a = {0, 0, 0, 0.0, 0, 0};
  for (uint64_t w = blocked ? ws.n : ws.first; w < ws.n; w += ws.stride) {
    const unsigned long long m = plane ? plane[w] : agg_keep_word(rows, w);  // (a row its condition does not pass is a row that is not kept)
    if (!m) continue;
    if (!EXPR && kind == AK_COUNT_ROWS) {  // (the word's popcount, once: lane 0's share)
      if (lane == 0) a.w0 += (unsigned long long)__builtin_popcountll(m);
      continue;
    }
    if (!((m >> lane) & 1)) continue;
    const FilterRow r = filter_row(rows, w * 64 + lane);
    if constexpr (EXPR) agg_expr_row<DIV, COND, CONV>(kind, ops + in.col, in.col2, rows.cols, r, rows.W, a);
    else agg_row(kind, is_max, in, c, c2, r, rows.W, a);
  }
  agg_block_fold(kind, is_max, a, fold_s);
  if (threadIdx.x == 0) agg_store(partials + (uint64_t)blockIdx.y * gridDim.x + blockIdx.x, a);
}
extern "C" __global__ void __launch_bounds__(256) agg_partial_kernel(const AggInsn* insns, KeptRows rows, AggPartial* partials) {
  __shared__ AggAcc fold_s[4];
  agg_partial_body<false>(insns, nullptr, rows, partials, fold_s);
}
extern "C" __global__ void __launch_bounds__(256) agg_expr_partial_kernel(const AggInsn* insns, const AggExprOp* ops, KeptRows rows, AggPartial* partials) {
  __shared__ AggAcc fold_s[4];
  agg_partial_body<true>(insns, ops, rows, partials, fold_s);
}
extern "C" __global__ void __launch_bounds__(256) agg_expr_div_partial_kernel(const AggInsn* insns, const AggExprOp* ops, KeptRows rows, AggPartial* partials) {
  __shared__ AggAcc fold_s[4];
  agg_partial_body<true, true>(insns, ops, rows, partials, fold_s);
}
// ... and the interpreter with the divide AND the conditionals (include/orcgpu.h: CONDITIONALS), launched in their place when a
// program of the list holds a conditional op (agg_ops_hold_conditional).  Resources: INTEGRATION.md 6p.
extern "C" __global__ void __launch_bounds__(256) agg_expr_cond_partial_kernel(const AggInsn* insns, const AggExprOp* ops, KeptRows rows, AggPartial* partials) {
  __shared__ AggAcc fold_s[4];
  agg_partial_body<true, true, true>(insns, ops, rows, partials, fold_s);
}
// ... and the mixed interpreter (include/orcgpu.h: CONVERSIONS), launched in their place when a program of the list holds a
// conversion (agg_ops_hold_conversion): it runs every program of the list.  Resources: INTEGRATION.md 6q.
extern "C" __global__ void __launch_bounds__(256) agg_expr_conv_partial_kernel(const AggInsn* insns, const AggExprOp* ops, KeptRows rows, AggPartial* partials) {
  __shared__ AggAcc fold_s[4];
  agg_partial_body<true, true, true, true>(insns, ops, rows, partials, fold_s);
}

// What a final kernel's block makes of n_blocks records that lie `stride` records apart: thread t folds records t, t + 256, ... in
// index order, then the block's tree -- that order is the contract.  Thread 0 holds the result.
__device__ __forceinline__ AggAcc agg_fold_records(uint32_t kind, bool is_max, const AggPartial* p, uint64_t stride, uint32_t n_blocks, AggAcc* fold_s) {
  AggAcc a = {0, 0, 0, 0.0, 0, 0};
  for (uint32_t k = threadIdx.x; k < n_blocks; k += 256) {
    const AggPartial& q = p[k * stride];
    const AggAcc b = {q.w[0], q.w[1], q.w[2], q.f, q.count, q.flags};
    agg_fold(kind, is_max, a, b);
  }
  agg_block_fold(kind, is_max, a, fold_s);
  return a;
}

// blockIdx.x = instruction: its n_blocks records -> out[instruction]
extern "C" __global__ void __launch_bounds__(256)
agg_final_kernel(const AggInsn* insns, const AggPartial* partials, uint32_t n_blocks, AggPartial* out) {
  __shared__ AggAcc fold_s[4];
  const AggInsn in = insns[blockIdx.x];
  const uint32_t kind = in.kind < AK_ALL_N ? in.kind : AK_COUNT_ROWS;
  const AggAcc a = agg_fold_records(kind, in.is_max != 0, partials + (uint64_t)blockIdx.x * n_blocks, 1, n_blocks, fold_s);
  if (threadIdx.x == 0) agg_store(out + blockIdx.x, a);
}
