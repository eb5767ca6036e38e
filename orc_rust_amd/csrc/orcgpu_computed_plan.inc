// orcgpu_computed_plan.inc -- computed columns (include/orcgpu.h: "Computed columns") as the host plans them, free of HIP and of the
// reader: the names checked against each other and against the file's root columns, each expression compiled by the expression
// compiler the aggregates and the row filter share (orcgpu_agg_expr.inc) in the mode a side of the row filter's comparison takes
// -- a Date is int64 days, the columns an expression cannot take are ORCGPU_UNSUPPORTED --, the output kind and scale fixed, the
// programs laid out one behind the other in ONE op table.  Every refusal of the computed columns is decided here and names the
// computed column.
#pragma once
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "orcgpu_agg_expr.inc"

namespace orcgpu_host {

struct ComputedColumn {
  std::string name;
  uint32_t cls = XCLASS_INT;  // XCLASS_*: Int64, Decimal128(38, scale), Float64
  int32_t scale = 0;          // XCLASS_DEC
  uint32_t first_op = 0, n_ops = 0;  // its program in ComputedPlan::ops
  std::vector<uint32_t> reads;       // the projected columns it reads, each once
};
struct ComputedPlan {
  std::vector<ComputedColumn> cols;
  std::vector<AggExprOp> ops;
  char err[384] = "";
};

// what a computed column is to everything that resolves names behind it: an ORC Long, Decimal(38, s) or Double
inline int32_t computed_orc_type(const ComputedColumn& c) { return c.cls == XCLASS_FLOAT ? ORCGPU_T_DOUBLE : c.cls == XCLASS_DEC ? ORCGPU_T_DECIMAL : ORCGPU_T_LONG; }
inline uint32_t computed_width(const ComputedColumn& c) { return c.cls == XCLASS_DEC ? 16 : 8; }

// The names alone: 1 .. ORCGPU_COMPUTED_MAX of them, non-empty, distinct, none a root column name of the file (file_roots: every
// root column, projected or not; none known yet: null, 0).  What the setter can refuse before the file's columns are known.
inline int computed_check_names(const char* const* names, uint32_t n, const char* const* file_roots, uint32_t n_file_roots, char* err, size_t err_len) {
  auto fail = [&](const char* fmt, const char* a = "") {
    snprintf(err, err_len, fmt, a);
    return (int)ORCGPU_INVALID_ARGUMENT;
  };
  if (!names || !n) return fail("computed columns: no computed column given");
  if (n > ORCGPU_COMPUTED_MAX) return fail("computed columns: more than ORCGPU_COMPUTED_MAX (8) computed columns");
  for (uint32_t k = 0; k < n; k++) {
    if (!names[k] || !names[k][0]) return fail("computed columns: a computed column without a name");
    for (uint32_t j = 0; j < k; j++)
      if (strcmp(names[j], names[k]) == 0) return fail("computed columns: the name '%s' is given twice", names[k]);
    for (uint32_t j = 0; j < n_file_roots; j++)
      if (file_roots[j] && strcmp(file_roots[j], names[k]) == 0) return fail("computed columns: '%s' is the name of a root column of the file", names[k]);
  }
  return ORCGPU_OK;
}

// names / exprs: the n computed columns as given.  file_roots: every root column name of the file, projected or not.
// proj_names / proj_cols: the projected root columns the expressions may read; proj_nested[k]: root k is a Struct / List / Map / Union.
inline int computed_compile(const char* const* names, const orcgpu_agg_expr* exprs, uint32_t n, const char* const* file_roots, uint32_t n_file_roots,
                            const char* const* proj_names, const AggExprCol* proj_cols, const uint8_t* proj_nested, uint32_t n_proj, ComputedPlan& plan) {
  plan.cols.clear();
  plan.ops.clear();
  plan.err[0] = 0;
  auto fail = [&](int rc, const char* fmt, const char* a = "", const char* b = "") {
    snprintf(plan.err, sizeof(plan.err), fmt, a, b);
    return rc;
  };
  if (!exprs) return fail(ORCGPU_INVALID_ARGUMENT, "computed columns: no computed column given");
  if (const int rc = computed_check_names(names, n, file_roots, n_file_roots, plan.err, sizeof(plan.err))) return rc;
  for (uint32_t j = 0; j < n_proj; j++)
    if (proj_nested && proj_nested[j])
      return fail(ORCGPU_UNSUPPORTED, "computed columns: the projected column '%s' is nested (Struct / List / Map / Union): not supported beside computed columns", proj_names[j]);
  for (uint32_t k = 0; k < n; k++) {
    const orcgpu_agg_expr& e = exprs[k];
    // an operand that is itself a computed column, and an expression without any column, are refused by name before the compiler
    // would call the first "not a projected root column"
    bool any_column = false;
    for (uint32_t x = 0; e.nodes && x < e.n_nodes && x < ORCGPU_AGG_EXPR_MAX_NODES; x++) {
      if (e.nodes[x].op != ORCGPU_AGG_EXPR_COLUMN || !e.nodes[x].column) continue;
      any_column = true;
      for (uint32_t j = 0; j < n; j++)
        if (strcmp(names[j], e.nodes[x].column) == 0)
          return fail(ORCGPU_UNSUPPORTED, "computed column '%s': its operand '%s' is a computed column: not supported", names[k], e.nodes[x].column);
    }
    char msg[256] = "";
    const std::string what = std::string("computed column '") + names[k] + "'";
    AggExprCompiler x{proj_names, proj_cols, n_proj, what.c_str(), msg, sizeof(msg)};
    x.predicate = true;
    ComputedColumn c;
    c.name = names[k];
    c.first_op = (uint32_t)plan.ops.size();
    uint32_t kind = 0;
    const int rc = x.compile(&e, plan.ops, kind, c.scale);
    if (rc) {
      plan.ops.resize(c.first_op);
      snprintf(plan.err, sizeof(plan.err), "%s", msg);
      return rc;
    }
    if (!any_column) {
      plan.ops.resize(c.first_op);
      return fail(ORCGPU_INVALID_ARGUMENT, "computed column '%s': its expression holds no column", names[k]);
    }
    c.cls = (uint32_t)x.cls;
    c.n_ops = (uint32_t)plan.ops.size() - c.first_op;
    // (a program with conditionals has no gates: its pushes name the columns; a program with gates pushes no other column)
    for (uint32_t o = c.first_op; o < plan.ops.size(); o++) {
      if (plan.ops[o].op > AX_PUSH_F64) continue;
      bool dup = false;
      for (const uint32_t seen : c.reads) dup |= seen == plan.ops[o].col;
      if (!dup) c.reads.push_back(plan.ops[o].col);
    }
    plan.cols.push_back(std::move(c));
  }
  return ORCGPU_OK;
}

}  // namespace orcgpu_host
