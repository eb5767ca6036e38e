// compute_kernels.hip -- computed columns (include/orcgpu.h: "Computed columns"): an arithmetic expression over decoded flat root
// columns, evaluated once per stripe into an ordinary fixed-width column of the result -- values and validity in the layout the
// decode leaves for every such column (filter_access.h), so that the row selection, the row filter, the aggregates, the top-k, the
// key-set insert and both exports read it as if the file had held it.
//
//   compute_columns_kernel     grid (ceil(n_batches * W / 4), computed columns) x 256.  blockIdx.y = the computed column (its
//                              ComputeJob).  A wavefront takes ONE validity word of the output: word w of uniform batch u, i.e.
//                              rows u * B + w * 64 + lane of the stripe.  A lane reads its row's operands through filter_access.h,
//                              runs the column's AggExprOp program with the interpreter of agg_expr_eval.h (the text the aggregates
//                              and the row filter run), stores the 8- or 16-byte value -- 0 for a NULL row -- and the wavefront's
//                              ballot of "valid" becomes the validity word, stored by lane 0.
//
// NULL: a gating operand is NULL (AGG_ROW_NULL).  NULL and counted: an operation left 128 bits (AGG_ROW_OVERFLOW), an Int64 result
// does not fit int64, a Decimal result has |value| >= 10^38.  Never a wrapped value.  Every row of the stripe gets its value; the
// COUNT is of the selected rows: with a row selection (count_all = 0) a row counts only when it lies in one of the selection's
// batches (SelBatch segments, ascending and disjoint, known before the decode call), found by a binary search over their starts.
//
// What may race: the batch's null count and the column's overflow count, integer adds of a wavefront's popcounts (a sum does not
// depend on their order).  No atomic decides a value or a place, and none is floating-point.  A value and a validity word are
// written by one lane, once.
// Bounds, each clamped here rather than trusted:
//   word index g = blockIdx.x * 4 + wavefront  < n_batches * W      (a wavefront past it leaves before it touches memory)
//   batch u = g / W                            < n_batches          (by the line above: the null count's slot, the validity word)
//   row l of the batch = (g % W) * 64 + lane   < B                  (a lane past it is dead: B need not be a multiple of 64)
//   row of the stripe = u * B + l              < n_rows             (a lane past it is dead)
//   a dead lane loads and stores nothing; a live lane's loads are at `row` of buffers of n_rows values and at validity word
//   u * W + l / 64 of n_batches * W words, its store at `row` of n_rows values of 8 or 16 bytes.
//   a segment index of the search stays below n_segs (lo <= hi < n_segs; n_segs = 0 is never searched); a segment is compared
//   with, never indexed with.
//   An operand index comes from the program, which the host compiled against the same column table; it is checked below n_cols
//   before the program runs (a job whose program names a column past the table writes NULLs and counts nothing).
// LDS: none.  Plain C++: no inline assembly.
//
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): in front of the kernel.
#pragma once
#include <stdint.h>

#include "agg_expr_eval.h"
#include "filter_access.h"
#include "select_kernels.hip"

enum { CK_INT64 = 0, CK_DEC128 = 1, CK_F64 = 2 };

// One computed column of one stripe
struct ComputeJob {
  const AggExprOp* prog;              // the column's program: its gates, then the post-order ops
  uint32_t n_ops;
  uint32_t kind;                      // CK_*
  uint8_t* out_values;                // n_rows values of 8 (CK_INT64, CK_F64) or 16 bytes (CK_DEC128)
  unsigned long long* out_validity;   // n_batches * W words
  unsigned long long* null_counts;    // n_batches counts, zero before the launch
  unsigned long long* overflow_rows;  // one count, zero before the launch
};

struct ComputeExprRow {
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

// gfx950: compute_columns_kernel VGPRs 55, SGPRs 90; compute_columns_div_kernel VGPRs 63, SGPRs 96; both LDS 0, scratch 0 (none
// expected, none used), occupancy 8 waves / SIMD
// (The body of two kernels: DIV = false is compute_columns_kernel; DIV = true, the interpreter with the divide, is
// compute_columns_div_kernel, launched in its place when a program of the plan holds a division.)
template <bool DIV, bool COND = false, bool CONV = false>
__device__ __forceinline__ void compute_columns_body(const ComputeJob* jobs, const FilterCol* cols, uint32_t n_cols, uint64_t n_rows, uint32_t n_batches, uint32_t B, uint32_t W,
                                                     const SelBatch* segs, uint32_t n_segs, uint32_t count_all) {
  const ComputeJob job = jobs[blockIdx.y];
  const uint64_t g = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= (uint64_t)n_batches * W) return;  // (the whole wavefront: the ballot below is taken by the wavefronts that stay)
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t u = g / W;
  const uint32_t l = (uint32_t)(g % W) * 64 + lane;
  const uint64_t row = u * B + l;
  const bool live = l < B && row < n_rows;
  // (uniform over the block: the program is the job's)
  bool sane = job.n_ops != 0;
  for (uint32_t k = 0; k < job.n_ops; k++) {
    const uint32_t op = job.prog[k].op;
    if (op <= AX_PUSH_F64 && job.prog[k].col >= n_cols) sane = false;
  }
  int state = AGG_ROW_NULL;
  agg_i128 iv = 0;
  double fv = 0.0;
  if (live && sane) {
    const ComputeExprRow x{cols, filter_row_of(row, B), W};
    if (job.kind == CK_F64) {
      state = agg_expr_eval_f64_as<DIV, COND, CONV>(job.prog, job.n_ops, x, &fv);
    } else {
      state = agg_expr_eval_i128_as<DIV, COND, CONV>(job.prog, job.n_ops, x, &iv);
      if (state == AGG_ROW_VALUE) {
        if (job.kind == CK_INT64) {
          if (iv != (agg_i128)(long long)iv) state = AGG_ROW_OVERFLOW;
        } else {
          const agg_i128 lim = agg_pow10(38);
          if (iv >= lim || iv <= -lim) state = AGG_ROW_OVERFLOW;
        }
      }
    }
  }
  const bool valid = state == AGG_ROW_VALUE;
  bool counted = state == AGG_ROW_OVERFLOW;
  if (counted && !count_all) {  // (rare: only an overflowed row searches) the last segment that starts at or before the row
    counted = false;
    if (n_segs) {
      uint32_t lo = 0, hi = n_segs - 1;
      while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (segs[mid].start <= row) lo = mid;
        else hi = mid - 1;
      }
      const SelBatch sb = segs[lo];
      counted = row >= sb.start && row - sb.start < sb.len;
    }
  }
  if (live) {
    if (job.kind == CK_DEC128) {
      const agg_u128 v = valid ? (agg_u128)iv : (agg_u128)0;
      uint4 q;
      q.x = (uint32_t)v;
      q.y = (uint32_t)(v >> 32);
      q.z = (uint32_t)(v >> 64);
      q.w = (uint32_t)(v >> 96);
      reinterpret_cast<uint4*>(job.out_values)[row] = q;
    } else if (job.kind == CK_F64) {
      reinterpret_cast<unsigned long long*>(job.out_values)[row] = valid ? agg_bits_of_f64(fv) : 0ull;
    } else {
      reinterpret_cast<long long*>(job.out_values)[row] = valid ? (long long)iv : 0ll;
    }
  }
  const unsigned long long m_valid = __ballot(valid), m_live = __ballot(live), m_over = __ballot(counted);
  if (lane == 0) {
    job.out_validity[g] = m_valid;
    const uint32_t nulls = (uint32_t)(__popcll(m_live) - __popcll(m_valid));
    if (nulls) atomicAdd(job.null_counts + u, (unsigned long long)nulls);
    if (m_over) atomicAdd(job.overflow_rows, (unsigned long long)__popcll(m_over));
  }
}
__global__ __launch_bounds__(256) void compute_columns_kernel(const ComputeJob* jobs, const FilterCol* cols, uint32_t n_cols, uint64_t n_rows, uint32_t n_batches,
                                                              uint32_t B, uint32_t W, const SelBatch* segs, uint32_t n_segs, uint32_t count_all) {
  compute_columns_body<false>(jobs, cols, n_cols, n_rows, n_batches, B, W, segs, n_segs, count_all);
}
__global__ __launch_bounds__(256) void compute_columns_div_kernel(const ComputeJob* jobs, const FilterCol* cols, uint32_t n_cols, uint64_t n_rows, uint32_t n_batches,
                                                                  uint32_t B, uint32_t W, const SelBatch* segs, uint32_t n_segs, uint32_t count_all) {
  compute_columns_body<true>(jobs, cols, n_cols, n_rows, n_batches, B, W, segs, n_segs, count_all);
}
// (the interpreter with the divide and the conditionals: launched when a program of the plan holds a conditional op)
__global__ __launch_bounds__(256) void compute_columns_cond_kernel(const ComputeJob* jobs, const FilterCol* cols, uint32_t n_cols, uint64_t n_rows, uint32_t n_batches,
                                                                   uint32_t B, uint32_t W, const SelBatch* segs, uint32_t n_segs, uint32_t count_all) {
  compute_columns_body<true, true>(jobs, cols, n_cols, n_rows, n_batches, B, W, segs, n_segs, count_all);
}
// (the mixed interpreter: launched when a program of the plan holds a conversion)
__global__ __launch_bounds__(256) void compute_columns_conv_kernel(const ComputeJob* jobs, const FilterCol* cols, uint32_t n_cols, uint64_t n_rows, uint32_t n_batches,
                                                                   uint32_t B, uint32_t W, const SelBatch* segs, uint32_t n_segs, uint32_t count_all) {
  compute_columns_body<true, true, true>(jobs, cols, n_cols, n_rows, n_batches, B, W, segs, n_segs, count_all);
}
