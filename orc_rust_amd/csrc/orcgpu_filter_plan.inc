// orcgpu_filter_plan.inc -- the row filter's plan compiler, host only and free of HIP (tests/hostcheck/filter_plan_check.cpp
// compiles this very text under AddressSanitizer + UBSan): a predicate as the pre-order node list of include/orcgpu.h ->
// the post-order program filter_eval_kernel runs (device/filter_program.h).  Names become column indices, the type table
// of orcgpu_result_filter is applied, and the depth is bounded.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "device/filter_program.h"

namespace orcgpu_host {

struct FilterPlan {
  std::vector<FilterInsn> prog;
  std::vector<uint8_t> lits;  // the string literals, one after the other
  uint32_t depth = 0;         // of the predicate (a leaf alone: 1)
  char err[256] = {0};
};

struct FilterCompiler {
  const orcgpu_predicate_node* nodes;
  uint32_t n_nodes;
  const char* const* names;
  const int32_t* kinds;  // ORCGPU_T_* of every column
  uint32_t n_columns;
  FilterPlan& out;

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
        const int kind = kinds[col], vt = n.value_type;
        const bool int_lit = vt == ORCGPU_PV_INT8 || vt == ORCGPU_PV_INT16 || vt == ORCGPU_PV_INT32 || vt == ORCGPU_PV_INT64;
        FilterInsn in{};
        in.cmp = (uint32_t)n.op;
        in.col = col;
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
          case ORCGPU_T_TIMESTAMP: case ORCGPU_T_TIMESTAMP_INSTANT: case ORCGPU_T_DECIMAL:
            return fail(ORCGPU_UNSUPPORTED, "row filter: a comparison on the Timestamp / Decimal column '%s' is not supported (IS [NOT] NULL is)", n.column);
          default:
            return fail(ORCGPU_UNSUPPORTED, "row filter: column '%s' of ORC type kind %lld cannot be compared", n.column, kind);
        }
        if (!ok) return fail(ORCGPU_MISMATCHED_SCHEMA, "row filter: column '%s' cannot be compared with a literal of value type %lld", n.column, vt);
        if (n.value_is_null) {
          emit(FOP_UNKNOWN);
          return ORCGPU_OK;
        }
        if (in.op == FOP_CMP_STRING) {
          if (n.s_len && !n.s) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the literal for column '%s' has a length and no bytes", n.column);
          if (n.s_len > 0x7fffffffull) return fail(ORCGPU_INVALID_ARGUMENT, "row filter: the literal for column '%s' is longer than 2^31 - 1 bytes", n.column);
          in.lit_off = out.lits.size();
          in.lit_len = (uint32_t)n.s_len;
          if (n.s_len) out.lits.insert(out.lits.end(), reinterpret_cast<const uint8_t*>(n.s), reinterpret_cast<const uint8_t*>(n.s) + n.s_len);
        }
        out.prog.push_back(in);
        return ORCGPU_OK;
      }
      default:
        return fail(ORCGPU_INVALID_ARGUMENT, "row filter: unknown node op%s %lld", "", n.op);
    }
  }
};

// ORCGPU_OK, or the status a reader with this filter ends with (out.err says why).  names[k] / kinds[k]: column k.
inline int filter_compile(const orcgpu_predicate_node* nodes, uint32_t n_nodes, const char* const* names, const int32_t* kinds, uint32_t n_columns,
                          FilterPlan& out) {
  out.prog.clear();
  out.lits.clear();
  out.depth = 0;
  out.err[0] = 0;
  FilterCompiler fc{nodes, n_nodes, names, kinds, n_columns, out};
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

}  // namespace orcgpu_host
