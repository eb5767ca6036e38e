// filter_expr_eval.h -- the comparison of an expression leaf of the row filter (include/orcgpu.h: ORCGPU_PRED_CMP_EXPR), ONE text
// for filter_expr_kernel (filter_kernels.hip), the host's plan compiler, which folds a leaf of two literal sides with it
// (orcgpu_filter_plan.inc), and the CPU check that runs it against Python ints and Fractions
// (tests/hostcheck/filter_plan_expr_check.cpp).  The two sides are evaluated by agg_expr_eval.h; what stands here is what happens
// to the two values: the order of two int128, of two doubles, and of two Decimals of differing scales.  Plain C++ behind AGG_HD.
#pragma once
#include <stdint.h>

#include "agg_expr_eval.h"
#include "filter_program.h"

// lt / eq / gt -> the operator's answer (cmp: ORCGPU_PRED_EQ .. _GE = 0 .. 5), as filter_eval_word spells it for its own leaves
AGG_HD bool filter_expr_answer(uint32_t cmp, bool lt, bool eq, bool gt) {
  switch (cmp) {
    case 0: return eq;
    case 1: return !eq;  // (true with a NaN on either side)
    case 2: return lt;
    case 3: return lt || eq;
    case 4: return gt;
    default: return gt || eq;
  }
}

// a OP b for two exact values.  d = b's scale minus a's (0 for the INT class), p10 = 10^|d|: the side of the smaller scale is
// multiplied by p10.  Where that product leaves 128 bits the order is decided by its sign alone: a positive value too large for an
// int128 is greater than any int128, a negative one smaller (it is not zero: zero times anything fits).
AGG_HD bool filter_expr_compare_i128(uint32_t cmp, agg_i128 a, agg_i128 b, int32_t d, agg_i128 p10) {
  bool lt, gt;
  if (d == 0) {
    lt = a < b;
    gt = a > b;
  } else if (d > 0) {  // b is the finer one: a * 10^d against b
    agg_i128 x = 0;
    if (agg_mul_checked(a, p10, &x)) {
      lt = x < b;
      gt = x > b;
    } else {
      lt = a < 0;
      gt = !lt;
    }
  } else {
    agg_i128 y = 0;
    if (agg_mul_checked(b, p10, &y)) {
      lt = a < y;
      gt = a > y;
    } else {
      gt = b < 0;
      lt = !gt;
    }
  }
  return filter_expr_answer(cmp, lt, !lt && !gt, gt);
}

// ... for two doubles, IEEE: with a NaN on either side all but NE are false, -0.0 == 0.0
AGG_HD bool filter_expr_compare_f64(uint32_t cmp, double a, double b) { return filter_expr_answer(cmp, a < b, a == b, a > b); }

// The header of a leaf's blob in the literal pool (filter_program.h), checked against the blob's length: false for what only a
// damaged upload holds
struct FilterExprBlob {
  uint32_t cls, n_lhs, n_rhs;
  int32_t d;
  agg_i128 p10;
  const AggExprOp *lhs, *rhs;
};
constexpr uint32_t kFilterExprMaxOps = 256;  // a side: at most 32 nodes, a power of ten and a gate for each
AGG_HD bool filter_expr_blob(const uint8_t* p, uint32_t len, FilterExprBlob* b) {
  if (len < kExprHeaderBytes) return false;
  const uint32_t* h = reinterpret_cast<const uint32_t*>(p);
  const unsigned long long* q = reinterpret_cast<const unsigned long long*>(p + 16);
  b->cls = h[0];
  b->n_lhs = h[1];
  b->n_rhs = h[2];
  b->d = (int32_t)h[3];
  b->p10 = agg_i128_of(q[0], q[1]);
  b->lhs = reinterpret_cast<const AggExprOp*>(p + kExprHeaderBytes);
  b->rhs = b->lhs + b->n_lhs;
  return b->cls <= FXC_FLOAT && b->n_lhs && b->n_rhs && b->n_lhs <= kFilterExprMaxOps && b->n_rhs <= kFilterExprMaxOps &&
         (uint64_t)kExprHeaderBytes + ((uint64_t)b->n_lhs + b->n_rhs) * kExprOpBytes <= len && b->d >= -38 && b->d <= 38;
}
