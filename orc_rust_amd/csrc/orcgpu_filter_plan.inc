// orcgpu_filter_plan.inc -- the row filter's plan compiler, host only and free of HIP (tests/hostcheck/filter_plan_check.cpp
// compiles this very text under AddressSanitizer + UBSan): a predicate as the pre-order node list of include/orcgpu.h ->
// the post-order program filter_eval_kernel runs (device/filter_program.h).  Names become column indices, the type table
// of orcgpu_result_filter is applied, Decimal128 and TimestampNs literals are brought to the column's own scale / unit, LIKE
// patterns are cut into the parts filter_like_kernel matches (tests/hostcheck/filter_plan_like_check.cpp), IN lists become the
// hash sets filter_in_kernel probes (orcgpu_in.inc, tests/hostcheck/filter_plan_in_check.cpp), the two sides of an expression leaf
// (lhs OP rhs) become the op tables filter_expr_kernel interprets -- compiled by the expression aggregates' compiler,
// orcgpu_agg_expr.inc (tests/hostcheck/filter_plan_expr_check.cpp) --, a set leaf (x IN SET s) becomes FOP_IN_SET with the address
// of the sealed table of the key set it names (orcgpu_key_set.inc, tests/hostcheck/key_set_check.cpp), and the depth is bounded.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device/filter_expr_eval.h"
#include "device/filter_program.h"
#include "orcgpu_agg_expr.inc"
#include "orcgpu_decimal.inc"
#include "orcgpu_in.inc"
#include "orcgpu_key_set.inc"
#include "orcgpu_like.inc"

namespace orcgpu_host {

static_assert(ORCGPU_PRED_IN == 17 && ORCGPU_PRED_LITERAL == 18 && ORCGPU_IN_MAX_VALUES == 65536, "the IN leaf of include/orcgpu.h");
static_assert(ORCGPU_PRED_CMP_EXPR == 19 && ORCGPU_PRED_EXPR_COLUMN == 20 && ORCGPU_PRED_EXPR_NEG == 25 &&
                  ORCGPU_PRED_EXPR_LITERAL - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_LITERAL && ORCGPU_PRED_EXPR_ADD - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_ADD &&
                  ORCGPU_PRED_EXPR_SUB - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_SUB && ORCGPU_PRED_EXPR_MUL - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_MUL &&
                  ORCGPU_PRED_EXPR_NEG - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_NEG && ORCGPU_PRED_EXPR_DATE_PART - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_DATE_PART &&
                  ORCGPU_PRED_EXPR_DIV - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_DIV && ORCGPU_PRED_EXPR_FLOOR_DIV - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_FLOOR_DIV &&
                  ORCGPU_PRED_EXPR_MOD - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_MOD && ORCGPU_PRED_EXPR_IF - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_IF &&
                  ORCGPU_PRED_EXPR_COALESCE - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_COALESCE && ORCGPU_PRED_EXPR_ABS - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_ABS &&
                  ORCGPU_PRED_EXPR_NULL - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_NULL && ORCGPU_PRED_EXPR_CMP - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_CMP &&
                  ORCGPU_PRED_EXPR_IS_NULL - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_IS_NULL && ORCGPU_PRED_EXPR_AND - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_AND &&
                  ORCGPU_PRED_EXPR_OR - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_OR && ORCGPU_PRED_EXPR_NOT - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_NOT &&
                  ORCGPU_PRED_EXPR_CAST - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_CAST && ORCGPU_PRED_EXPR_TRUNC - ORCGPU_PRED_EXPR_COLUMN == ORCGPU_AGG_EXPR_TRUNC,
              "the expression leaf of include/orcgpu.h: its nodes are the expression aggregates', 20 further on");
static_assert((int)FXC_INT == (int)XCLASS_INT && (int)FXC_DEC == (int)XCLASS_DEC && (int)FXC_FLOAT == (int)XCLASS_FLOAT && sizeof(AggExprOp) == kExprOpBytes, "filter_program.h: an expression leaf's blob");
static_assert(kLikeMaxBytes == ORCGPU_LIKE_MAX_BYTES && kLikeMaxParts == ORCGPU_LIKE_MAX_PARTS, "the LIKE limits of include/orcgpu.h are the kernel's");

struct FilterPlan {
  std::vector<FilterInsn> prog;
  std::vector<uint8_t> lits;  // the string literals, one after the other
  uint32_t depth = 0;         // of the predicate (a leaf alone: 1)
  // the leaves with a mask plane, as instruction indices in program order: the grids of filter_like_kernel and filter_in_kernel
  // ... and of filter_expr_kernel.  A LIKE and an IN leaf own one plane, an expression leaf TWO (T, then F; neither bit: UNKNOWN)
  std::vector<uint32_t> like_leaves, in_leaves, expr_leaves;
  size_t n_planes() const { return like_leaves.size() + in_leaves.size() + 2 * expr_leaves.size(); }  // (numbered together, in leaf order: FilterInsn::i)
  size_t n_leaves() const { return like_leaves.size() + in_leaves.size() + expr_leaves.size(); }
  // the memory of the key sets whose tables FOP_IN_SET instructions name by address: whoever keeps the plan keeps them alive
  std::vector<std::shared_ptr<void>> holds;
  char err[256] = {0};
};

struct FilterCompiler {
  const orcgpu_predicate_node* nodes;
  uint32_t n_nodes;
  const char* const* names;
  const int32_t* kinds;  // ORCGPU_T_* of every column
  uint32_t n_columns;
  const int32_t* params;  // per column -- Decimal: its scale; Timestamp: the unit it is decoded to (0 s, 1 ms, 2 us, 3 ns, 4 Decimal128(38, 9))
  FilterPlan& out;
  const KeySetRefs* sets = nullptr;  // the key sets of the context the plan is compiled for (none: every set leaf is refused)

  int fail(int rc, const char* fmt, const char* a = "", long long b = 0) {
    snprintf(out.err, sizeof(out.err), fmt, a, b);
    return rc;
  }
  int column(const orcgpu_predicate_node& n, uint32_t& col) {
    if (!n.column) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: a leaf without a column name%s (node op %lld)", "", n.op);
    for (uint32_t k = 0; k < n_columns; k++)
      if (names[k] && strcmp(names[k], n.column) == 0) {
        col = k;
        return ORCGPU_OK;
      }
    return fail(ORCGPU_INVALID_ARGUMENT, "row filter: column '%s' is not a projected root column", n.column);
  }
  void emit(uint32_t op, uint32_t cmp = 0, uint32_t col = 0) {
    FilterInsn in{};
    in.op = op;
    in.cmp = cmp;
    in.col = col;
    out.prog.push_back(in);
  }
  // the bytes of a string literal: there when it has a length, and few enough for an int32 offset
  int check_bytes(const char* s, uint64_t s_len, const char* column) {
    if (s_len && !s) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the literal for column '%s' has a length and no bytes", column);
    if (s_len > 0x7fffffffull) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the literal for column '%s' is longer than 2^31 - 1 bytes", column);
    return ORCGPU_OK;
  }
  // ... checked and appended to the literal pool, as the literal of instruction `in`
  int pool_bytes(const char* s, uint64_t s_len, const char* column, FilterInsn& in) {
    if (const int rc = check_bytes(s, s_len, column)) return rc;
    in.lit_off = out.lits.size();
    in.lit_len = (uint32_t)s_len;
    if (s_len) out.lits.insert(out.lits.end(), reinterpret_cast<const uint8_t*>(s), reinterpret_cast<const uint8_t*>(s) + s_len);
    return ORCGPU_OK;
  }
  // the instruction about to be pushed takes the next mask plane and joins its kernel's leaf list
  void take_plane(FilterInsn& in, std::vector<uint32_t>& leaves) {
    in.i = (long long)out.n_planes();
    leaves.push_back((uint32_t)out.prog.size());
  }
  // A Decimal128 literal -> (op', literal') at the column's own scale, so that the kernel compares unscaled values and never
  // rescales a row.  d = column scale - literal scale.  d >= 0: literal * 10^d, clamped to int128 where it leaves it -- no valid
  // Decimal (|v| < 10^38 < 2^127) equals a clamp, so EQ is never TRUE and the order comparisons are right as they stand.
  // d < 0: q = floor(literal / 10^-d); with a remainder no row equals the literal: EQ / NE are asked of the upper clamp (still
  // UNKNOWN on a null row), LT / LE become LE q, GT / GE become GT q.
  int decimal(const orcgpu_predicate_node& n, const char* column, uint32_t col, FilterInsn& in) {
    i128 lit = 0;
    if (!dec_literal(n.s, n.s_len, n.i, lit))
      return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the Decimal128 literal for column '%s' is malformed (16 bytes, a scale of 0 .. 38, a magnitude below 10^38)", column);
    return decimal_value(lit, (int)n.i, column, col, in);
  }
  // ... the literal as a value: |lit| < 10^38 at lit_scale 0 .. 38
  int decimal_value(i128 lit, int lit_scale, const char* column, uint32_t col, FilterInsn& in) {
    const int col_scale = params ? params[col] : 0;
    if (col_scale < 0 || col_scale > kDecMaxDigits) return fail(ORCGPU_UNSUPPORTED, "row filter: the Decimal column '%s' has the scale %lld", column, col_scale);
    const int d = col_scale - lit_scale;
    i128 L = 0;
    if (d >= 0) {
      if (!dec_scale_up(lit, d, L)) L = lit < 0 ? dec_i128_min() : dec_i128_max();
    } else {
      bool exact = false;
      dec_floor_div(lit, -d, L, exact);
      if (!exact) {
        if (in.cmp == ORCGPU_PRED_EQ || in.cmp == ORCGPU_PRED_NE) L = dec_i128_max();
        else in.cmp = in.cmp == ORCGPU_PRED_LT || in.cmp == ORCGPU_PRED_LE ? ORCGPU_PRED_LE : ORCGPU_PRED_GT;
      }
    }
    in.i = (long long)(L >> 64);
    in.lo = (unsigned long long)L;
    return ORCGPU_OK;
  }
  // A TimestampNs literal -> (op', literal') in the unit the column is decoded to: q = floor(ns / unit), as above.  The literal is
  // in the finest unit, so it is only ever divided and nothing can leave int64.  Every int64 is a value a row may hold, hence the
  // constant cases are asked of INT64_MIN: LT is TRUE for no valid row, GE for every one, both UNKNOWN on a null row.
  int timestamp(const orcgpu_predicate_node& n, const char* column, uint32_t col, FilterInsn& in) {
    static const int64_t per_unit[4] = {1000000000, 1000000, 1000, 1};  // seconds, milli-, micro-, nanoseconds
    const int unit = params ? params[col] : 3;
    if (unit < 0 || unit > 3)
      return fail(ORCGPU_UNSUPPORTED, "row filter: the Timestamp column '%s' is decoded to Decimal128(38, 9), not to an int64 unit: a comparison on it is not supported", column);
    const int64_t p = per_unit[unit];
    int64_t q = n.i / p, r = n.i % p;
    if (r < 0) {  // (C++ truncates toward zero; instants before 1970 need the floor)
      q -= 1;
      r += p;
    }
    if (r) {
      if (in.cmp == ORCGPU_PRED_EQ || in.cmp == ORCGPU_PRED_NE) {
        in.cmp = in.cmp == ORCGPU_PRED_EQ ? ORCGPU_PRED_LT : ORCGPU_PRED_GE;
        q = INT64_MIN;
      } else in.cmp = in.cmp == ORCGPU_PRED_LT || in.cmp == ORCGPU_PRED_LE ? ORCGPU_PRED_LE : ORCGPU_PRED_GT;
    }
    in.i = q;
    return ORCGPU_OK;
  }
  // The type table of orcgpu_result_filter: may the literal of node `n` be compared with column `col` (named `column`)?  Sets the
  // instruction's class and, for the plain kinds, its literal.  A comparison and every literal of an IN list go through here.
  int literal(const orcgpu_predicate_node& n, const char* column, uint32_t col, FilterInsn& in) {
    const int kind = kinds[col], vt = n.value_type;
    const bool int_lit = vt == ORCGPU_PV_INT8 || vt == ORCGPU_PV_INT16 || vt == ORCGPU_PV_INT32 || vt == ORCGPU_PV_INT64;
    bool ok = false;
    switch (kind) {
      case ORCGPU_T_BYTE: case ORCGPU_T_SHORT: case ORCGPU_T_INT: case ORCGPU_T_LONG:
        ok = int_lit;
        in.op = FOP_CMP_INT;
        in.i = n.i;
        break;
      case ORCGPU_T_DATE:
        ok = vt == ORCGPU_PV_INT32 || vt == ORCGPU_PV_INT64;
        in.op = FOP_CMP_INT;
        in.i = n.i;
        break;
      case ORCGPU_T_FLOAT: case ORCGPU_T_DOUBLE:
        ok = vt == ORCGPU_PV_FLOAT32 || vt == ORCGPU_PV_FLOAT64;
        in.op = FOP_CMP_FLOAT;
        in.f = vt == ORCGPU_PV_FLOAT32 ? (double)(float)n.f : n.f;
        break;
      case ORCGPU_T_BOOLEAN:
        ok = vt == ORCGPU_PV_BOOLEAN;
        in.op = FOP_CMP_BOOL;
        in.i = n.i != 0;
        break;
      case ORCGPU_T_STRING: case ORCGPU_T_VARCHAR: case ORCGPU_T_CHAR: case ORCGPU_T_BINARY:
        ok = vt == ORCGPU_PV_UTF8;
        in.op = FOP_CMP_STRING;
        break;
      case ORCGPU_T_DECIMAL:
        if (vt != ORCGPU_PV_DECIMAL128)
          return fail(ORCGPU_UNSUPPORTED, "row filter: the Decimal column '%s' is compared with Decimal128 literals only (value type %lld is not supported)", column, vt);
        ok = true;
        in.op = FOP_CMP_DEC128;
        break;
      case ORCGPU_T_TIMESTAMP: case ORCGPU_T_TIMESTAMP_INSTANT:
        if (vt != ORCGPU_PV_TIMESTAMP_NS)
          return fail(ORCGPU_UNSUPPORTED, "row filter: the Timestamp column '%s' is compared with TimestampNs literals only (value type %lld is not supported)", column, vt);
        ok = true;
        in.op = FOP_CMP_INT;
        break;
      default:
        return fail(ORCGPU_UNSUPPORTED, "row filter: column '%s' of ORC type kind %lld cannot be compared", column, kind);
    }
    if (!ok) return fail(ORCGPU_MISMATCHED_SCHEMA, "row filter: column '%s' cannot be compared with a literal of value type %lld", column, vt);
    return ORCGPU_OK;
  }
  // the node at `at` and everything below it; `at` then stands behind them
  int node(uint32_t& at, uint32_t depth) {
    if (at >= n_nodes) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the node list ends inside a node's children%s (%lld nodes)", "", n_nodes);
    if (depth > ORCGPU_FILTER_MAX_DEPTH) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the predicate is deeper than %s%lld levels", "", ORCGPU_FILTER_MAX_DEPTH);
    if (depth > out.depth) out.depth = depth;
    const orcgpu_predicate_node& n = nodes[at++];
    switch (n.op) {
      case ORCGPU_PRED_AND:
      case ORCGPU_PRED_OR: {
        const uint32_t op = n.op == ORCGPU_PRED_AND ? FOP_AND : FOP_OR;
        if (!n.n_children) {
          emit(op == FOP_AND ? FOP_TRUE : FOP_FALSE);
          return ORCGPU_OK;
        }
        for (uint32_t k = 0; k < n.n_children; k++) {
          const int rc = node(at, depth + 1);
          if (rc) return rc;
          if (k) emit(op);
        }
        return ORCGPU_OK;
      }
      case ORCGPU_PRED_NOT: {
        const int rc = node(at, depth + 1);
        if (rc) return rc;
        emit(FOP_NOT);
        return ORCGPU_OK;
      }
      case ORCGPU_PRED_IS_NULL:
      case ORCGPU_PRED_IS_NOT_NULL: {
        uint32_t col = 0;
        const int rc = column(n, col);
        if (rc) return rc;
        emit(n.op == ORCGPU_PRED_IS_NULL ? FOP_IS_NULL : FOP_IS_NOT_NULL, 0, col);
        return ORCGPU_OK;
      }
      case ORCGPU_PRED_EQ: case ORCGPU_PRED_NE: case ORCGPU_PRED_LT: case ORCGPU_PRED_LE: case ORCGPU_PRED_GT: case ORCGPU_PRED_GE: {
        uint32_t col = 0;
        const int rc = column(n, col);
        if (rc) return rc;
        const int kind = kinds[col];
        FilterInsn in{};
        in.cmp = (uint32_t)n.op;
        in.col = col;
        if (const int lrc = literal(n, n.column, col, in)) return lrc;
        if (n.value_is_null) {
          emit(FOP_UNKNOWN);
          return ORCGPU_OK;
        }
        if (kind == ORCGPU_T_DECIMAL) {
          if (const int drc = decimal(n, n.column, col, in)) return drc;
        } else if (kind == ORCGPU_T_TIMESTAMP || kind == ORCGPU_T_TIMESTAMP_INSTANT) {
          if (const int trc = timestamp(n, n.column, col, in)) return trc;
        }
        if (in.op == FOP_CMP_STRING)
          if (const int src = pool_bytes(n.s, n.s_len, n.column, in)) return src;
        out.prog.push_back(in);
        return ORCGPU_OK;
      }
      case ORCGPU_PRED_LIKE: {
        uint32_t col = 0;
        const int rc = column(n, col);
        if (rc) return rc;
        return like(n, col);
      }
      case ORCGPU_PRED_IN: {
        // (the shape of the list before anything else: its literal nodes follow the leaf, and `at` must end behind them)
        if ((uint64_t)at + n.n_children > n_nodes)
          return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the node list ends inside an IN list%s (%lld nodes)", "", n_nodes);
        for (uint32_t k = 0; k < n.n_children; k++) {
          const orcgpu_predicate_node& l = nodes[at + k];
          if (l.op != ORCGPU_PRED_LITERAL)
            return fail(ORCGPU_INVALID_ARGUMENT, "row filter: an IN list holds literal nodes only%s (node op %lld)", "", l.op);
          if (l.n_children) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: a literal node of an IN list has children%s (%lld)", "", l.n_children);
        }
        uint32_t col = 0;
        const int rc = column(n, col);
        if (rc) return rc;
        const int irc = in_list(n, nodes + at, col);
        at += n.n_children;
        return irc;
      }
      case ORCGPU_PRED_CMP_EXPR:
        return cmp_expr(n, at);
      case ORCGPU_PRED_IN_SET: {
        uint32_t col = 0;
        const int rc = column(n, col);
        if (rc) return rc;
        return in_set(n, col);
      }
      case ORCGPU_PRED_EXPR_COLUMN: case ORCGPU_PRED_EXPR_LITERAL: case ORCGPU_PRED_EXPR_ADD: case ORCGPU_PRED_EXPR_SUB: case ORCGPU_PRED_EXPR_MUL: case ORCGPU_PRED_EXPR_NEG:
      case ORCGPU_PRED_EXPR_DATE_PART: case ORCGPU_PRED_EXPR_DIV: case ORCGPU_PRED_EXPR_FLOOR_DIV: case ORCGPU_PRED_EXPR_MOD:
      case ORCGPU_PRED_EXPR_IF: case ORCGPU_PRED_EXPR_COALESCE: case ORCGPU_PRED_EXPR_ABS: case ORCGPU_PRED_EXPR_NULL: case ORCGPU_PRED_EXPR_CMP:
      case ORCGPU_PRED_EXPR_IS_NULL: case ORCGPU_PRED_EXPR_AND: case ORCGPU_PRED_EXPR_OR: case ORCGPU_PRED_EXPR_NOT:
      case ORCGPU_PRED_EXPR_CAST: case ORCGPU_PRED_EXPR_ROUND: case ORCGPU_PRED_EXPR_FLOOR: case ORCGPU_PRED_EXPR_CEIL: case ORCGPU_PRED_EXPR_TRUNC:
        return fail(ORCGPU_INVALID_ARGUMENT, "row filter: an expression node stands outside an expression comparison%s (node %lld)", "", (long long)at - 1);
      case ORCGPU_PRED_LITERAL:
        return fail(ORCGPU_INVALID_ARGUMENT, "row filter: a literal node stands outside an IN list%s (node %lld)", "", (long long)at - 1);
      default:
        return fail(ORCGPU_INVALID_ARGUMENT, "row filter: unknown node op%s %lld", "", n.op);
    }
  }
  // One side of an expression leaf: the subtree at `at` as the expression aggregates' nodes; `at` then stands behind it
  int expr_side(uint32_t& at, std::vector<orcgpu_agg_expr_node>& side) {
    if (at >= n_nodes) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the node list ends inside an expression%s (%lld nodes)", "", n_nodes);
    const orcgpu_predicate_node& n = nodes[at++];
    uint32_t kids = 0;
    switch (n.op) {
      case ORCGPU_PRED_EXPR_COLUMN: case ORCGPU_PRED_EXPR_LITERAL: kids = 0; break;
      case ORCGPU_PRED_EXPR_ADD: case ORCGPU_PRED_EXPR_SUB: case ORCGPU_PRED_EXPR_MUL: kids = 2; break;
      case ORCGPU_PRED_EXPR_DIV: case ORCGPU_PRED_EXPR_FLOOR_DIV: case ORCGPU_PRED_EXPR_MOD: kids = 2; break;  // (a division's scale travels in `i`, below)
      case ORCGPU_PRED_EXPR_NEG: case ORCGPU_PRED_EXPR_DATE_PART: kids = 1; break;  // (the part travels in `i`, below)
      // the conditionals (the comparison of a CMP travels in `i`); numbers against conditions are the expression compiler's to check
      case ORCGPU_PRED_EXPR_IF: kids = 3; break;
      case ORCGPU_PRED_EXPR_COALESCE: case ORCGPU_PRED_EXPR_CMP: case ORCGPU_PRED_EXPR_AND: case ORCGPU_PRED_EXPR_OR: kids = 2; break;
      case ORCGPU_PRED_EXPR_ABS: case ORCGPU_PRED_EXPR_IS_NULL: case ORCGPU_PRED_EXPR_NOT: kids = 1; break;
      case ORCGPU_PRED_EXPR_NULL: kids = 0; break;
      // the conversions (a CAST's target travels in value_type and `i`, a ROUND's digits in `i`, below)
      case ORCGPU_PRED_EXPR_CAST: case ORCGPU_PRED_EXPR_ROUND: case ORCGPU_PRED_EXPR_FLOOR: case ORCGPU_PRED_EXPR_CEIL: case ORCGPU_PRED_EXPR_TRUNC: kids = 1; break;
      default: return fail(ORCGPU_INVALID_ARGUMENT, "row filter: an expression holds expression nodes only%s (node op %lld)", "", n.op);
    }
    if (n.n_children != kids) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: an expression node with the wrong number of children%s (%lld)", "", n.n_children);
    if (n.op == ORCGPU_PRED_EXPR_LITERAL && n.value_is_null)
      return fail(ORCGPU_INVALID_ARGUMENT, "row filter: an expression holds no NULL literal%s (node %lld)", "", (long long)at - 1);
    if (side.size() > ORCGPU_AGG_EXPR_MAX_NODES) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: a side of an expression comparison has more than ORCGPU_AGG_EXPR_MAX_NODES (%s%lld) nodes", "", ORCGPU_AGG_EXPR_MAX_NODES);
    orcgpu_agg_expr_node x{};
    x.op = (uint32_t)(n.op - ORCGPU_PRED_EXPR_COLUMN);
    x.column = n.column;
    x.value_type = n.value_type;
    x.i = n.i;
    x.f = n.f;
    x.s = n.s;
    x.s_len = n.s_len;
    side.push_back(x);
    for (uint32_t k = 0; k < kids; k++)
      if (const int rc = expr_side(at, side)) return rc;
    return ORCGPU_OK;
  }
  static uint32_t mirrored(uint32_t cmp) {  // a OP b == b OP' a
    return cmp == ORCGPU_PRED_LT ? ORCGPU_PRED_GT : cmp == ORCGPU_PRED_GT ? ORCGPU_PRED_LT : cmp == ORCGPU_PRED_LE ? ORCGPU_PRED_GE : cmp == ORCGPU_PRED_GE ? ORCGPU_PRED_LE : cmp;
  }
  // An expression leaf, lhs OP rhs (include/orcgpu.h).  Both sides are compiled by the expression aggregates' compiler, typed
  // together; then by shape: two literals: TRUE / FALSE; a bare column against a literal its own comparison takes: that comparison,
  // mirrored when the column is on the right; everything else: FOP_CMP_EXPR with the two op tables in the literal pool and two
  // mask planes.
  int cmp_expr(const orcgpu_predicate_node& n, uint32_t& at) {
    if (n.n_children != 2) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: an expression comparison has two sides%s (%lld children)", "", n.n_children);
    if (n.i < ORCGPU_PRED_EQ || n.i > ORCGPU_PRED_GE) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the operator of an expression comparison is %s%lld (ORCGPU_PRED_EQ .. _GE: 0 .. 5)", "", n.i);
    std::vector<orcgpu_agg_expr_node> ln, rn;
    if (const int rc = expr_side(at, ln)) return rc;
    if (const int rc = expr_side(at, rn)) return rc;
    std::vector<AggExprCol> xcols(n_columns);
    for (uint32_t k = 0; k < n_columns; k++) {
      AggExprCol& c = xcols[k];
      c.orc_type = kinds[k];
      const int cls = agg_class(kinds[k]);
      c.scale = cls == ACLASS_DEC && params && params[k] > 0 ? (uint32_t)params[k] : 0;
      // (what the decode made of the column is checked against the compiled leaf per call: filter_check_kinds)
      c.fkind = cls == ACLASS_FLOAT ? FKIND_FLOAT : cls == ACLASS_DEC ? FKIND_DEC128 : (cls == ACLASS_INT || cls == ACLASS_DATE) ? FKIND_INT : FKIND_OTHER;
    }
    AggExprCompiler x{names, xcols.data(), n_columns, "a comparison", out.err, sizeof(out.err)};
    x.predicate = true;
    const orcgpu_agg_expr le{ln.data(), (uint32_t)ln.size()}, re{rn.data(), (uint32_t)rn.size()};
    AggExprCompiler::Side l, r;
    if (const int rc = x.compile_pair(&le, &re, l, r)) {
      // (the compiler's messages speak for the aggregates: here it is the row filter that refuses)
      std::string msg = out.err;
      if (msg.compare(0, 10, "aggregate:") == 0) msg = "row filter:" + msg.substr(10);
      snprintf(out.err, sizeof(out.err), "%s", msg.c_str());
      return rc;
    }
    const uint32_t cmp = (uint32_t)n.i;
    const int32_t d = x.cls == XCLASS_DEC ? r.scale - l.scale : 0;  // (both 0 .. 38)
    const agg_i128 p10 = agg_pow10((uint32_t)(d < 0 ? -d : d));
    if (l.is_lit && r.is_lit) {
      const bool t = x.cls == XCLASS_FLOAT ? filter_expr_compare_f64(cmp, l.fv, r.fv) : filter_expr_compare_i128(cmp, l.iv, r.iv, d, p10);
      emit(t ? FOP_TRUE : FOP_FALSE);
      return ORCGPU_OK;
    }
    if ((l.is_col && r.is_lit) || (l.is_lit && r.is_col)) {
      const AggExprCompiler::Side &c = l.is_col ? l : r, &v = l.is_col ? r : l;
      const int kind = agg_class(kinds[c.col]);
      FilterInsn in{};
      in.cmp = l.is_col ? cmp : mirrored(cmp);
      in.col = c.col;
      if (x.cls == XCLASS_FLOAT) {
        in.op = FOP_CMP_FLOAT;
        in.f = v.fv;
        out.prog.push_back(in);
        return ORCGPU_OK;
      }
      if (x.cls == XCLASS_INT && v.iv >= (agg_i128)INT64_MIN && v.iv <= (agg_i128)INT64_MAX) {
        in.op = FOP_CMP_INT;
        in.i = (long long)v.iv;
        out.prog.push_back(in);
        return ORCGPU_OK;
      }
      const agg_i128 lim = dec_pow10(kDecMaxDigits);
      if (x.cls == XCLASS_DEC && kind == ACLASS_DEC && v.iv > -lim && v.iv < lim && v.scale >= 0 && v.scale <= kDecMaxDigits) {
        in.op = FOP_CMP_DEC128;
        if (const int rc = decimal_value(v.iv, v.scale, names[c.col], c.col, in)) return rc;
        out.prog.push_back(in);
        return ORCGPU_OK;
      }
    }
    FilterInsn in{};
    in.op = FOP_CMP_EXPR;
    in.cmp = cmp;
    in.i = (long long)out.n_planes();  // its T plane; i + 1: its F plane
    out.expr_leaves.push_back((uint32_t)out.prog.size());
    while (out.lits.size() & 7) out.lits.push_back(0);
    in.lit_off = out.lits.size();
    const size_t n_ops = l.ops.size() + r.ops.size();
    out.lits.resize(in.lit_off + kExprHeaderBytes + n_ops * sizeof(AggExprOp));
    put32(out.lits, in.lit_off, (uint32_t)x.cls);
    put32(out.lits, in.lit_off + 4, (uint32_t)l.ops.size());
    put32(out.lits, in.lit_off + 8, (uint32_t)r.ops.size());
    put32(out.lits, in.lit_off + 12, (uint32_t)d);
    const unsigned long long pw[2] = {(unsigned long long)p10, (unsigned long long)((agg_u128)p10 >> 64)};
    memcpy(out.lits.data() + in.lit_off + 16, pw, 16);
    memcpy(out.lits.data() + in.lit_off + kExprHeaderBytes, l.ops.data(), l.ops.size() * sizeof(AggExprOp));
    memcpy(out.lits.data() + in.lit_off + kExprHeaderBytes + l.ops.size() * sizeof(AggExprOp), r.ops.data(), r.ops.size() * sizeof(AggExprOp));
    in.lit_len = (uint32_t)(out.lits.size() - in.lit_off);
    out.prog.push_back(in);
    return ORCGPU_OK;
  }
  // A LIKE leaf.  The pattern is cut at its unescaped `%` into parts of literal bytes and `_` marks; since a `_` takes exactly the
  // code point that stands there, a part matched from a given start has one length and the kernel never backtracks: the first part
  // sits at the value's start unless the pattern begins with `%`, the last one at its end unless it ends with `%`, the ones
  // between are found leftmost-first.  No wildcard: the string comparison EQ; only `%`: every valid row.
  int like(const orcgpu_predicate_node& n, uint32_t col) {
    const int kind = kinds[col];
    if ((kind != ORCGPU_T_STRING && kind != ORCGPU_T_VARCHAR && kind != ORCGPU_T_CHAR) || n.value_type != ORCGPU_PV_UTF8)
      return fail(ORCGPU_MISMATCHED_SCHEMA, "row filter: LIKE takes a String / Varchar / Char column and a Utf8 pattern: column '%s' with value type %lld does not fit", n.column, n.value_type);
    if (n.i < 0 || n.i > 127) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the LIKE escape for column '%s' is %lld (0: none, else 1 .. 127)", n.column, n.i);
    if (n.value_is_null) {
      emit(FOP_UNKNOWN);
      return ORCGPU_OK;
    }
    if (n.s_len && !n.s) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the LIKE pattern for column '%s' has a length and no bytes", n.column);
    if (n.s_len > 2ull * kLikeMaxBytes)  // (even with every byte escaped)
      return fail(ORCGPU_UNSUPPORTED, "row filter: the LIKE pattern for column '%s' is longer than %lld bytes", n.column, kLikeMaxBytes);
    LikePattern pat;
    if (!like_unescape(n.s, (size_t)n.s_len, (int)n.i, pat))
      return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the LIKE pattern for column '%s' ends in its escape byte", n.column);
    const size_t ne = pat.kinds.size();
    if (ne > kLikeMaxBytes)
      return fail(ORCGPU_UNSUPPORTED, "row filter: the LIKE pattern for column '%s' is longer than %lld bytes", n.column, kLikeMaxBytes);
    FilterInsn in{};
    in.col = col;
    if (pat.wildcard_free()) {
      in.op = FOP_CMP_STRING;
      in.cmp = ORCGPU_PRED_EQ;
      if (const int src = pool_bytes(reinterpret_cast<const char*>(pat.bytes.data()), ne, n.column, in)) return src;
      out.prog.push_back(in);
      return ORCGPU_OK;
    }
    std::vector<uint32_t> part_first, part_len;
    std::vector<uint8_t> bytes, ones;
    bool any_one = false;
    for (size_t k = 0; k < ne;) {
      if (pat.kinds[k] == LIKE_EL_ANY) {
        k++;
        continue;
      }
      part_first.push_back((uint32_t)bytes.size());
      for (; k < ne && pat.kinds[k] != LIKE_EL_ANY; k++) {
        bytes.push_back(pat.bytes[k]);
        ones.push_back(pat.kinds[k] == LIKE_EL_ONE);
        any_one |= pat.kinds[k] == LIKE_EL_ONE;
      }
      part_len.push_back((uint32_t)bytes.size() - part_first.back());
    }
    const uint32_t np = (uint32_t)part_first.size();
    if (np > kLikeMaxParts)
      return fail(ORCGPU_UNSUPPORTED, "row filter: the LIKE pattern for column '%s' has more than %lld parts between its %% signs", n.column, kLikeMaxParts);
    const uint32_t flags = (pat.kinds[0] != LIKE_EL_ANY ? LIKE_ANCHOR_START : 0) | (pat.kinds[ne - 1] != LIKE_EL_ANY ? LIKE_ANCHOR_END : 0);
    uint32_t shape = LIKE_GENERAL;
    if (!np) shape = LIKE_ALL;
    else if (np == 1 && !any_one) shape = flags == LIKE_ANCHOR_START ? LIKE_PREFIX : flags == LIKE_ANCHOR_END ? LIKE_SUFFIX : flags == 0 ? LIKE_CONTAINS : LIKE_GENERAL;
    in.op = FOP_LIKE;
    in.cmp = shape;
    if (shape != LIKE_ALL) {
      take_plane(in, out.like_leaves);  // its plane of match bits
      while (out.lits.size() & 3) out.lits.push_back(0);
      in.lit_off = out.lits.size();
      std::vector<uint32_t> words = {shape, flags, np, (uint32_t)bytes.size()};
      for (uint32_t p = 0; p < np; p++) {
        words.push_back(part_first[p]);
        words.push_back(part_len[p]);
      }
      out.lits.resize(in.lit_off + 4 * words.size());
      for (size_t w = 0; w < words.size(); w++) put32(out.lits, in.lit_off + 4 * w, words[w]);
      out.lits.insert(out.lits.end(), bytes.begin(), bytes.end());
      out.lits.insert(out.lits.end(), ones.begin(), ones.end());
      in.lit_len = (uint32_t)(out.lits.size() - in.lit_off);
    }
    out.prog.push_back(in);
    return ORCGPU_OK;
  }
  // A set leaf: x IN SET s is x IN (the keys the set's build side held, NULLs included), so by the IN list's shapes: an empty set
  // without a NULL: FALSE; an empty one with: UNKNOWN; everything else: FOP_IN_SET -- FOP_IN whose table is the set's own, sealed on
  // the device and named by address, with a mask plane among the IN leaves' (filter_in_kernel's grid takes both).  The keys never
  // come to the host, so one key is not turned into an EQ.
  int in_set(const orcgpu_predicate_node& n, uint32_t col) {
    if (n.n_children) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the set leaf for column '%s' has children (%lld)", n.column, n.n_children);
    if (const int rc = key_set_column_check(kinds[col], false, false, n.column, "row filter", out.err, sizeof(out.err))) return rc;
    const KeySetRef* set = nullptr;
    for (size_t k = 0; sets && k < sets->size(); k++)
      if ((*sets)[k].id == (uint64_t)n.i) set = &(*sets)[k];
    if (!set) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the key set named for column '%s' (id %lld) is not a set of this context", n.column, n.i);
    if (set->state == KEY_SET_BUILDING) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the key set named for column '%s' (id %lld) is not sealed", n.column, n.i);
    if (set->state != KEY_SET_SEALED)
      return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the key set named for column '%s' took more than its limit of %lld keys and is unusable", n.column, set->max_keys);
    if (!set->n_keys) {
      emit(set->has_null ? FOP_UNKNOWN : FOP_FALSE);
      return ORCGPU_OK;
    }
    FilterInsn in{};
    in.op = FOP_IN_SET;
    in.col = col;
    in.cmp = set->has_null ? IN_HAS_NULL : 0;
    in.lo = FKIND_INT;
    take_plane(in, out.in_leaves);
    in.lit_off = set->table;
    in.lit_len = set->bytes;
    out.holds.push_back(set->hold);
    out.prog.push_back(in);
    return ORCGPU_OK;
  }
  // An IN leaf: x IN (v1 .. vk) is OR(x = v1, ..., x = vk).  Every literal passes the type table of EQ and is brought to the
  // column's key by the code EQ uses; a literal that can equal no row (NaN, a Decimal off the column's scale, a Timestamp between
  // two values of its unit) is FALSE on valid rows like the empty rest of the OR, so it is left out.  Then by shape: no literal:
  // FALSE; only NULLs, or no usable key beside a NULL: UNKNOWN; one key and no NULL: the EQ instruction itself; a Boolean column
  // and a list without a usable key: FOP_IN without a table; everything else: FOP_IN with a hash set and a mask plane.
  int in_list(const orcgpu_predicate_node& n, const orcgpu_predicate_node* list, uint32_t col) {
    const uint32_t k = n.n_children;
    if (k > ORCGPU_IN_MAX_VALUES)
      return fail(ORCGPU_UNSUPPORTED, "row filter: the IN list for column '%s' holds more than %lld values", n.column, ORCGPU_IN_MAX_VALUES);
    if (!k) {
      emit(FOP_FALSE);
      return ORCGPU_OK;
    }
    const int kind = kinds[col];
    const bool is_ts = kind == ORCGPU_T_TIMESTAMP || kind == ORCGPU_T_TIMESTAMP_INSTANT;
    InKeys keys;
    uint32_t fop = 0;
    uint64_t bytes = 0;
    bool has_false = false, has_true = false;
    for (uint32_t x = 0; x < k; x++) {
      const orcgpu_predicate_node& l = list[x];
      FilterInsn eq{};
      eq.cmp = ORCGPU_PRED_EQ;
      eq.col = col;
      if (const int lrc = literal(l, n.column, col, eq)) return lrc;
      fop = eq.op;
      if (l.value_is_null) {
        keys.has_null = true;
        continue;
      }
      if (eq.op == FOP_CMP_INT) {
        if (is_ts) {
          if (const int trc = timestamp(l, n.column, col, eq)) return trc;
          if (eq.cmp != ORCGPU_PRED_EQ) continue;  // between two values of the unit
        }
        keys.k64.push_back((uint64_t)eq.i);
      } else if (eq.op == FOP_CMP_FLOAT) {
        if (eq.f != eq.f) continue;  // NaN
        keys.k64.push_back(in_float_key(eq.f));
      } else if (eq.op == FOP_CMP_BOOL) {
        (eq.i ? has_true : has_false) = true;
      } else if (eq.op == FOP_CMP_DEC128) {
        if (const int drc = decimal(l, n.column, col, eq)) return drc;
        const i128 v = (i128)(((unsigned __int128)(uint64_t)eq.i << 64) | (unsigned __int128)eq.lo), lim = dec_pow10(kDecMaxDigits);
        if (v <= -lim || v >= lim) continue;  // off the column's scale, or beyond every Decimal
        keys.add_dec128(eq.lo, eq.i);
      } else {
        if (const int src = check_bytes(l.s, l.s_len, n.column)) return src;
        bytes += l.s_len;
        if (bytes > ORCGPU_IN_MAX_BYTES)
          return fail(ORCGPU_UNSUPPORTED, "row filter: the IN list for column '%s' holds more than %lld bytes of literals", n.column, ORCGPU_IN_MAX_BYTES);
        keys.kstr.emplace_back(l.s ? l.s : "", (size_t)l.s_len);
      }
    }
    keys.kind = fop == FOP_CMP_DEC128 ? IN_KEY_DEC128 : fop == FOP_CMP_STRING ? IN_KEY_STRING : IN_KEY_I64;
    keys.dedup();
    const size_t nk = fop == FOP_CMP_BOOL ? (size_t)has_false + has_true : keys.size();
    if (!nk && keys.has_null) {
      emit(FOP_UNKNOWN);
      return ORCGPU_OK;
    }
    FilterInsn in{};
    in.col = col;
    if (nk == 1 && !keys.has_null) {  // the comparison itself: no plane, no further kernel
      in.op = fop;
      in.cmp = ORCGPU_PRED_EQ;
      if (fop == FOP_CMP_BOOL) in.i = has_true;
      else if (fop == FOP_CMP_INT) in.i = (long long)keys.k64[0];
      else if (fop == FOP_CMP_FLOAT) memcpy(&in.f, &keys.k64[0], 8);
      else if (fop == FOP_CMP_DEC128) {
        in.i = InKeys::dec_high(keys.k128[0]);
        in.lo = keys.k128[0].second;
      } else if (const int src = pool_bytes(keys.kstr[0].data(), keys.kstr[0].size(), n.column, in)) return src;
      out.prog.push_back(in);
      return ORCGPU_OK;
    }
    in.op = FOP_IN;
    in.cmp = keys.has_null ? IN_HAS_NULL : 0;
    in.lo = fop_value_kind(fop);
    if (!nk || fop == FOP_CMP_BOOL) {
      in.cmp |= IN_NO_TABLE | (has_false ? IN_BOOL_FALSE : 0) | (has_true ? IN_BOOL_TRUE : 0);
      in.i = -1;
    } else {
      take_plane(in, out.in_leaves);
      in.lit_off = in_build_table(keys, in.cmp, out.lits, in.lit_len);
    }
    out.prog.push_back(in);
    return ORCGPU_OK;
  }
};

// ORCGPU_OK, or the status a reader with this filter ends with (out.err says why).  names[k] / kinds[k]: column k.
// params[k]: a Decimal column's scale, the unit a Timestamp column is decoded to (FilterCompiler::params); none: scale 0, nanoseconds.
inline int filter_compile(const orcgpu_predicate_node* nodes, uint32_t n_nodes, const char* const* names, const int32_t* kinds, uint32_t n_columns,
                          FilterPlan& out, const int32_t* params = nullptr, const KeySetRefs* sets = nullptr) {
  out.prog.clear();
  out.lits.clear();
  out.like_leaves.clear();
  out.in_leaves.clear();
  out.expr_leaves.clear();
  out.holds.clear();
  out.depth = 0;
  out.err[0] = 0;
  FilterCompiler fc{nodes, n_nodes, names, kinds, n_columns, params, out, sets};
  if (!nodes || !n_nodes) return fc.fail(ORCGPU_INVALID_ARGUMENT, "row filter: no predicate%s", "");
  for (uint32_t k = 0; k < n_columns; k++) {
    const int t = kinds[k];
    if (t == ORCGPU_T_STRUCT || t == ORCGPU_T_LIST || t == ORCGPU_T_MAP || t == ORCGPU_T_UNION)
      return fc.fail(ORCGPU_UNSUPPORTED, "row filter: the projection holds the nested column '%s' (Struct / List / Map / Union are not filtered)", names[k] ? names[k] : "");
  }
  uint32_t at = 0;
  const int rc = fc.node(at, 1);
  if (rc) return rc;
  if (at != n_nodes) return fc.fail(ORCGPU_INVALID_ARGUMENT, "row filter: %s%lld nodes are left behind the predicate's root", "", (long long)(n_nodes - at));
  return ORCGPU_OK;
}

// The columns whose VALUES an expression leaf reads (its gates read validity alone), each with the FKIND_* it must be decoded to:
// what fop_reads_values / fop_value_kind say of the other leaves, for a leaf that names several columns.  A gate's column is
// listed too, with kind FKIND_OTHER + 1 ("any"): it must exist.
struct FilterExprRead {
  uint32_t col, kind;
};
constexpr uint32_t kFilterExprAnyKind = FKIND_DEC128 + 1;
inline void filter_expr_reads(const FilterPlan& plan, const FilterInsn& in, std::vector<FilterExprRead>& out) {
  FilterExprBlob b;
  if (in.op != FOP_CMP_EXPR || in.lit_off > plan.lits.size() || in.lit_len > plan.lits.size() - in.lit_off || !filter_expr_blob(plan.lits.data() + in.lit_off, in.lit_len, &b)) return;
  for (uint32_t k = 0; k < b.n_lhs + b.n_rhs; k++) {
    AggExprOp op;
    memcpy(&op, plan.lits.data() + in.lit_off + kExprHeaderBytes + (size_t)k * sizeof(AggExprOp), sizeof(op));
    if (op.op == AX_GATE) out.push_back({op.col, kFilterExprAnyKind});
    else if (op.op == AX_PUSH_INT) out.push_back({op.col, FKIND_INT});
    else if (op.op == AX_PUSH_DEC) out.push_back({op.col, FKIND_DEC128});
    else if (op.op == AX_PUSH_F64) out.push_back({op.col, FKIND_FLOAT});
  }
}

// Does an expression leaf of the plan hold an op `holds` says yes to?
inline bool filter_plan_holds(const FilterPlan& plan, bool (*holds)(const AggExprOp*, size_t)) {
  for (const uint32_t leaf : plan.expr_leaves) {
    if (leaf >= plan.prog.size()) continue;
    const FilterInsn& in = plan.prog[leaf];
    FilterExprBlob b;
    if (in.op != FOP_CMP_EXPR || in.lit_off > plan.lits.size() || in.lit_len > plan.lits.size() - in.lit_off || !filter_expr_blob(plan.lits.data() + in.lit_off, in.lit_len, &b)) continue;
    for (uint32_t k = 0; k < b.n_lhs + b.n_rhs; k++) {
      AggExprOp op;
      memcpy(&op, plan.lits.data() + in.lit_off + kExprHeaderBytes + (size_t)k * sizeof(AggExprOp), sizeof(op));
      if (holds(&op, 1)) return true;
    }
  }
  return false;
}
// ... a division?  (The call then launches filter_expr_div_kernel in place of filter_expr_kernel.)
inline bool filter_plan_holds_division(const FilterPlan& plan) { return filter_plan_holds(plan, agg_ops_hold_division); }
// ... a conditional?  (filter_expr_cond_kernel, which has the divide too.)
inline bool filter_plan_holds_conditional(const FilterPlan& plan) { return filter_plan_holds(plan, agg_ops_hold_conditional); }
// ... a conversion?  (filter_expr_conv_kernel, the mixed interpreter.)
inline bool filter_plan_holds_conversion(const FilterPlan& plan) { return filter_plan_holds(plan, agg_ops_hold_conversion); }

// `from`, a plan compiled on its own against the same columns, behind `into`: its instructions behind into's, its literals behind
// into's from an 8-byte boundary (what the IN tables and the LIKE patterns are aligned to), its mask planes numbered behind
// into's, its leaves in into's leaf lists -- so that one literal pool, one launch of filter_like_kernel and one of filter_in_kernel
// serve both.  Returns the index of its first instruction.  This is how the conditions of an aggregate list (orcgpu_agg_plan.inc)
// share a program with each other and, at the call, with the row filter.
inline uint32_t filter_plan_append(FilterPlan& into, const FilterPlan& from) {
  const uint32_t first = (uint32_t)into.prog.size();
  const long long planes = (long long)into.n_planes();
  while (into.lits.size() & 7) into.lits.push_back(0);
  const unsigned long long lit0 = into.lits.size();
  into.lits.insert(into.lits.end(), from.lits.begin(), from.lits.end());
  for (FilterInsn in : from.prog) {
    if (in.op == FOP_CMP_STRING || in.op == FOP_LIKE || in.op == FOP_IN || in.op == FOP_CMP_EXPR) in.lit_off += lit0;
    // (a set leaf names its table by address: nothing of it lies in the pool)
    if ((in.op == FOP_LIKE && in.cmp != LIKE_ALL) || (in.op == FOP_IN && !(in.cmp & IN_NO_TABLE)) || in.op == FOP_IN_SET || in.op == FOP_CMP_EXPR) in.i += planes;
    into.prog.push_back(in);
  }
  for (const uint32_t k : from.like_leaves) into.like_leaves.push_back(first + k);
  for (const uint32_t k : from.in_leaves) into.in_leaves.push_back(first + k);
  for (const uint32_t k : from.expr_leaves) into.expr_leaves.push_back(first + k);
  into.holds.insert(into.holds.end(), from.holds.begin(), from.holds.end());
  if (from.depth > into.depth) into.depth = from.depth;
  return first;
}

}  // namespace orcgpu_host
