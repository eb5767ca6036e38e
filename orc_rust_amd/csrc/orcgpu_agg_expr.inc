// orcgpu_agg_expr.inc -- an aggregate's arithmetic expression (include/orcgpu.h: orcgpu_agg_expr) -> the post-order program the
// kernels interpret per kept row (device/agg_program.h: AggExprOp; device/agg_expr_eval.h), free of HIP
// (tests/hostcheck/agg_expr_check.cpp compiles this very text under AddressSanitizer + UBSan).  The pre-order nodes are parsed into
// a tree; the tree is typed (INT / DEC / FLOAT), the Decimal scale rule applied -- the operand of lower scale of a + b is wrapped
// into a multiplication by a power of ten --, a date part (year(d), ...) typed as an integer over an operand of days, subtrees of
// literals alone folded with the evaluator's own checked arithmetic and calendar function, the nodes labelled with the operand
// slots they need (Sethi-Ullman: the child that needs more goes first) and emitted.  Division (a / b, a // b, a % b; include/
// orcgpu.h: DIVISION): a `/` anywhere makes an exact expression a Decimal one, its node's scale and the power of ten of its dividend
// are decided with the scales; `//` and `%` take integers -- scale 0 -- and no doubles; where the right child of one of the three goes
// first, ONE AX_SWAP stands in front of the op (there are no reversed forms).  Conditionals (IF, COALESCE, ABS, NULL and the
// conditions CMP, IS_NULL, AND, OR, NOT; include/orcgpu.h: CONDITIONALS): numbers and conditions are told apart after the parse, the
// value operands of IF / COALESCE and the sides of CMP get the scale rule of +, the ternary node its own labelling, and a program
// that holds one is emitted WITHOUT gates, its column pushes nullable, behind a mark that makes every interpreter without the
// conditionals overflow the row (agg_program.h: kAggCondMark) -- a program that holds none is, op for op, what it was.  Conversions
// (CAST, ROUND, FLOOR, CEIL, TRUNC; include/orcgpu.h: CONVERSIONS): a tree that holds one (`mixed`) has its classes decided PER NODE,
// bottom-up (Node::nc: node_class, meet), each conversion node becomes the child itself, a folded literal or one of kToF64 ..
// kF64Round (type_conversion), and the program is laid out like one with conditionals, for the mixed interpreter alone, behind a
// mark and in front of a tail that keep it safe everywhere else (agg_program.h: kAggConvMarkCol) -- a tree that holds none takes
// none of these paths.  Every refusal of the expression aggregates is
// decided here.  Included from orcgpu_agg_plan.inc, in front of its compiler.
//
// The row filter's expression leaf (ORCGPU_PRED_CMP_EXPR: lhs OP rhs) has its two sides compiled here too (compile_pair, called by
// orcgpu_filter_plan.inc): one parse, one typing, one scale rule, one folding and one labelling for both users.  What differs is
// said by `predicate`: the class is decided over both sides together, a Date column takes part as int64 days, a side may hold no
// column at all, and the columns an expression cannot take are ORCGPU_UNSUPPORTED.  The file is self-contained: it describes a
// column by what the typing needs (AggExprCol), not by what the aggregates know of it.
#pragma once
#include <cstdio>
#include <cstring>
#include <vector>

#include "device/agg_expr_eval.h"
#include "device/filter_program.h"
#include "orcgpu_decimal.inc"

namespace orcgpu_host {

enum { ACLASS_INT, ACLASS_DATE, ACLASS_BOOL, ACLASS_FLOAT, ACLASS_DEC, ACLASS_TS, ACLASS_OTHER };
inline int agg_class(int32_t t) {
  switch (t) {
    case ORCGPU_T_BYTE: case ORCGPU_T_SHORT: case ORCGPU_T_INT: case ORCGPU_T_LONG: return ACLASS_INT;
    case ORCGPU_T_DATE: return ACLASS_DATE;
    case ORCGPU_T_BOOLEAN: return ACLASS_BOOL;
    case ORCGPU_T_FLOAT: case ORCGPU_T_DOUBLE: return ACLASS_FLOAT;
    case ORCGPU_T_DECIMAL: return ACLASS_DEC;
    case ORCGPU_T_TIMESTAMP: case ORCGPU_T_TIMESTAMP_INSTANT: return ACLASS_TS;
    default: return ACLASS_OTHER;
  }
}

// What the typing reads of a column
struct AggExprCol {
  int32_t orc_type = 0;
  uint32_t scale = 0;            // Decimal
  uint32_t fkind = FKIND_OTHER;  // FKIND_*: what the decode makes of its values
  bool dict_out = false;         // read as a dictionary column
  bool ts_wide = false;          // a Timestamp decoded to Decimal128(38, 9)
};

static_assert(sizeof(AggExprOp) == 24, "agg_program.h: the record the kernels read");
static_assert((int)AX_PART_YEAR == (int)ORCGPU_DATE_PART_YEAR && (int)AX_PART_DAY_OF_YEAR == (int)ORCGPU_DATE_PART_DAY_OF_YEAR && (int)AX_PART_N == (int)ORCGPU_DATE_PART_DAY_OF_YEAR + 1,
              "the parts of include/orcgpu.h are the interpreter's");
static_assert(ORCGPU_AGG_EXPR_DIV == 17 && ORCGPU_AGG_EXPR_FLOOR_DIV == 18 && ORCGPU_AGG_EXPR_MOD == 19, "the division nodes of include/orcgpu.h");
static_assert(ORCGPU_AGG_EXPR_IF == 21 && ORCGPU_AGG_EXPR_COALESCE == 22 && ORCGPU_AGG_EXPR_ABS == 23 && ORCGPU_AGG_EXPR_NULL == 24 && ORCGPU_AGG_EXPR_CMP == 25 &&
                  ORCGPU_AGG_EXPR_IS_NULL == 26 && ORCGPU_AGG_EXPR_AND == 27 && ORCGPU_AGG_EXPR_OR == 28 && ORCGPU_AGG_EXPR_NOT == 29,
              "the conditional nodes of include/orcgpu.h: the value nodes, then the condition nodes, without a gap");
static_assert(ORCGPU_AGG_EXPR_CAST == 30 && ORCGPU_AGG_EXPR_ROUND == 31 && ORCGPU_AGG_EXPR_FLOOR == 32 && ORCGPU_AGG_EXPR_CEIL == 33 && ORCGPU_AGG_EXPR_TRUNC == 34,
              "the conversion nodes of include/orcgpu.h, behind the conditionals without a gap");
static_assert(kAggExprSlots == ORCGPU_AGG_EXPR_MAX_DEPTH && kAggExprMaxNodes == ORCGPU_AGG_EXPR_MAX_NODES, "the limits of include/orcgpu.h");

enum { XCLASS_INT = 0, XCLASS_DEC = 1, XCLASS_FLOAT = 2 };

struct AggExprCompiler {
  const char* const* names;
  const AggExprCol* cols;
  uint32_t n_columns;
  const char* op_name;
  char* err;
  size_t err_len;
  bool predicate = false;  // the two sides of a row filter's expression leaf (the head comment)

  struct Node {
    uint32_t op = 0;        // ORCGPU_AGG_EXPR_*, or kScale: this library's own "times 10^k"
    int a = -1, b = -1;     // children
    int c = -1;             // IF: the third child (a: the condition, b: then, c: otherwise)
    uint32_t cmp = 0;       // CMP: ORCGPU_PRED_EQ .. _GE
    uint32_t col = 0;       // COLUMN
    int32_t value_type = 0; // LITERAL
    agg_i128 iv = 0;        // LITERAL of the INT / DEC class; kScale: 10^k
    double fv = 0.0;        // LITERAL of the FLOAT class
    int scale = 0;          // DEC
    uint32_t k = 0;         // kScale
    uint32_t part = 0;      // DATE_PART: ORCGPU_DATE_PART_*
    int want_scale = -1;    // DIV: the result scale the caller chose (the node's `i`), -1: the default rule
    bool in_date = false;   // a leaf that stands below a DATE_PART: its value is a number of days
    int nc = XCLASS_INT;    // a tree with conversions: the node's own class (XCLASS_*), decided bottom-up
    bool fop = false;       // ... and whether the node's OPERANDS are doubles (an arithmetic node, NEG, ABS, CMP): kAggOpF64
    int to = 0;             // CAST: the target class; its scale in want_scale.  ROUND: the digits in want_scale
    uint32_t label = 1;     // operand slots the subtree needs
  };
  static constexpr uint32_t kScale = 100;
  // ... and what a conversion node becomes once its child's class is known (type_node): one child each
  static constexpr uint32_t kToF64 = 101;     // exact at scale k -> double (AX_TO_F64)
  static constexpr uint32_t kF64ToDec = 102;  // double -> Decimal at scale k (AX_F64_TO_DEC)
  static constexpr uint32_t kF64ToInt = 103;  // double -> int64 (AX_F64_TO_INT)
  static constexpr uint32_t kRescale = 104;   // exact, divided by 10^k by the mode in `part` (AX_RESCALE)
  static constexpr uint32_t kToInt = 105;     // exact at scale k -> int64: AX_RESCALE by 10^k toward zero where k != 0, then AX_FIT_I64
  static constexpr uint32_t kF64Round = 106;  // double, rounded by the mode in `part` (AX_F64_ROUND)
  bool mixed = false;  // the tree holds a conversion node: classes are per node (Node::nc), and the program is one for the mixed interpreter
  std::vector<Node> t;
  const orcgpu_agg_expr_node* src = nullptr;
  uint32_t n_src = 0, at = 0;
  const char* first_column = "";
  int cls = XCLASS_INT;
  uint32_t date_depth = 0;      // parse: the DATE_PART nodes above the node at hand
  uint32_t date_part_of = 0;    // ... and the part of the innermost one, for the messages

  static bool is_division(uint32_t op) { return op == ORCGPU_AGG_EXPR_DIV || op == ORCGPU_AGG_EXPR_FLOOR_DIV || op == ORCGPU_AGG_EXPR_MOD; }
  static const char* division_name(uint32_t op) { return op == ORCGPU_AGG_EXPR_DIV ? "/" : op == ORCGPU_AGG_EXPR_FLOOR_DIV ? "//" : "%"; }
  // the conditional nodes (include/orcgpu.h: CONDITIONALS): those that produce a condition, and all nine
  static bool is_condition(uint32_t op) { return op >= ORCGPU_AGG_EXPR_CMP && op <= ORCGPU_AGG_EXPR_NOT; }
  static bool is_conditional(uint32_t op) { return op >= ORCGPU_AGG_EXPR_IF && op <= ORCGPU_AGG_EXPR_NOT; }
  static uint32_t conditional_children(uint32_t op) {
    return op == ORCGPU_AGG_EXPR_IF ? 3 : op == ORCGPU_AGG_EXPR_NULL ? 0 : (op == ORCGPU_AGG_EXPR_ABS || op == ORCGPU_AGG_EXPR_IS_NULL || op == ORCGPU_AGG_EXPR_NOT) ? 1 : 2;
  }
  // the conversion nodes (include/orcgpu.h: CONVERSIONS): one child each
  static bool is_conversion(uint32_t op) { return op >= ORCGPU_AGG_EXPR_CAST && op <= ORCGPU_AGG_EXPR_TRUNC; }
  static const char* node_name(uint32_t op) {
    static const char* const n[] = {"IF", "COALESCE", "ABS", "NULL", "CMP", "IS_NULL", "AND", "OR", "NOT", "CAST", "ROUND", "FLOOR", "CEIL", "TRUNC"};
    if (is_conditional(op) || is_conversion(op)) return n[op - ORCGPU_AGG_EXPR_IF];
    return op == ORCGPU_AGG_EXPR_COLUMN ? "a column" : op == ORCGPU_AGG_EXPR_LITERAL ? "a literal" : op == ORCGPU_AGG_EXPR_ADD ? "+" : op == ORCGPU_AGG_EXPR_SUB ? "-"
         : op == ORCGPU_AGG_EXPR_MUL ? "*" : op == ORCGPU_AGG_EXPR_NEG ? "unary -" : op == ORCGPU_AGG_EXPR_DATE_PART ? "a date part" : is_division(op) ? division_name(op) : "?";
  }
  static const char* part_name(uint32_t part) {
    static const char* const n[] = {"year()", "quarter()", "month()", "day()", "day_of_week()", "day_of_year()"};
    return part < AX_PART_N ? n[part] : "?";
  }

  int fail(int rc, const char* fmt, const char* a = "", const char* b = "", const char* c = "", const char* d = "") {
    snprintf(err, err_len, fmt, a, b, c, d);
    return rc;
  }

  // pre-order -> tree; `node` gets the subtree's root
  int parse(int& node) {
    if (at >= n_src) return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: the expression of %s ends before an operator has its operands", op_name);
    const orcgpu_agg_expr_node& s = src[at++];
    Node n;
    n.op = s.op;
    n.in_date = date_depth != 0;
    n.part = date_part_of;  // (a leaf: the function it stands below)
    const int me = (int)t.size();
    t.push_back(n);
    if (s.op == ORCGPU_AGG_EXPR_COLUMN) {
      if (!s.column) return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: a column node of the expression of %s without a name", op_name);
      uint32_t col = n_columns;
      for (uint32_t k = 0; k < n_columns && col == n_columns; k++)
        if (names[k] && strcmp(names[k], s.column) == 0) col = k;
      if (col == n_columns) return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: column '%s' in the expression of %s is not a projected root column", s.column, op_name);
      t[me].col = col;
      if (!*first_column) first_column = names[col];
    } else if (s.op == ORCGPU_AGG_EXPR_LITERAL) {
      t[me].value_type = s.value_type;
      if (s.value_type == ORCGPU_PV_INT64) {
        t[me].iv = s.i;
      } else if (s.value_type == ORCGPU_PV_FLOAT64) {
        t[me].fv = s.f;
      } else if (s.value_type == ORCGPU_PV_DECIMAL128) {
        i128 v = 0;
        if (!dec_literal(s.s, s.s_len, s.i, v)) return -1;  // (named below, once the first column is known)
        t[me].iv = v;
        t[me].scale = (int)s.i;
      } else {
        return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: a literal of the expression of %s is not an INT64, FLOAT64 or DECIMAL128 value", op_name);
      }
    } else if (s.op == ORCGPU_AGG_EXPR_ADD || s.op == ORCGPU_AGG_EXPR_SUB || s.op == ORCGPU_AGG_EXPR_MUL || s.op == ORCGPU_AGG_EXPR_NEG || is_division(s.op)) {
      if (s.op == ORCGPU_AGG_EXPR_DIV) {
        if (s.i < -1 || s.i > 38)
          return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: a division node of the expression of %s names no result scale (i: 0 .. 38, or -1 for the default rule)", op_name);
        t[me].want_scale = (int)s.i;
      }
      int a = -1, b = -1;
      if (const int rc = parse(a)) return rc;
      if (s.op != ORCGPU_AGG_EXPR_NEG)
        if (const int rc = parse(b)) return rc;
      t[me].a = a;
      t[me].b = b;
    } else if (s.op == ORCGPU_AGG_EXPR_DATE_PART) {
      if (s.i < ORCGPU_DATE_PART_YEAR || s.i > ORCGPU_DATE_PART_DAY_OF_YEAR)
        return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: a date part node of the expression of %s names no part (ORCGPU_DATE_PART_YEAR .. _DAY_OF_YEAR: 0 .. 5)", op_name);
      const uint32_t outer = date_part_of;
      date_depth++;
      date_part_of = (uint32_t)s.i;
      int a = -1;
      const int rc = parse(a);
      date_depth--;
      date_part_of = outer;
      if (rc) return rc;
      t[me].a = a;
      t[me].part = (uint32_t)s.i;
    } else if (is_conversion(s.op)) {
      if (s.op == ORCGPU_AGG_EXPR_CAST) {
        // (The message begins with the words an unknown node is refused in: until there was a CAST, 30 WAS an unknown node, a node 30
        // with nothing filled in -- value_type 0 -- is what a caller of that time sent, and tests/test_cond_host_sanitized.py pins
        // those words for it.  Same status as ever; the second half says what is wrong to a caller who did write a CAST.)
        if (s.value_type != ORCGPU_PV_INT64 && s.value_type != ORCGPU_PV_FLOAT64 && s.value_type != ORCGPU_PV_DECIMAL128)
          return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: an unknown node in the expression of %s: a CAST whose value_type names no target type (ORCGPU_PV_INT64, _FLOAT64 or _DECIMAL128)", op_name);
        if (s.value_type == ORCGPU_PV_DECIMAL128 && (s.i < 0 || s.i > 38))
          return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: a CAST node of the expression of %s to DECIMAL128 names no scale (i: 0 .. 38)", op_name);
        t[me].to = s.value_type == ORCGPU_PV_INT64 ? XCLASS_INT : s.value_type == ORCGPU_PV_FLOAT64 ? XCLASS_FLOAT : XCLASS_DEC;
        t[me].want_scale = s.value_type == ORCGPU_PV_DECIMAL128 ? (int)s.i : 0;
      } else if (s.op == ORCGPU_AGG_EXPR_ROUND) {
        if (s.i < 0 || s.i > 38) return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: a ROUND node of the expression of %s names no digits (i: 0 .. 38)", op_name);
        t[me].want_scale = (int)s.i;
      }
      mixed = true;
      // (what stands below a conversion is no operand of the date part above it: the node's own result is)
      const uint32_t outer_depth = date_depth;
      date_depth = 0;
      int a = -1;
      const int rc = at >= n_src ? fail(ORCGPU_INVALID_ARGUMENT, "aggregate: a %s node of the expression of %s stands without its child", node_name(s.op), op_name) : parse(a);
      date_depth = outer_depth;
      if (rc) return rc;
      t[me].a = a;
    } else if (is_conditional(s.op)) {
      if (s.op == ORCGPU_AGG_EXPR_CMP) {
        if (s.i < ORCGPU_PRED_EQ || s.i > ORCGPU_PRED_GE)
          return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: a CMP node of the expression of %s names no comparison (i: ORCGPU_PRED_EQ .. _GE, 0 .. 5)", op_name);
        t[me].cmp = (uint32_t)s.i;
      }
      int kid[3] = {-1, -1, -1};
      for (uint32_t k = 0; k < conditional_children(s.op); k++)
        if (const int rc = parse(kid[k])) return rc;
      t[me].a = kid[0];
      t[me].b = kid[1];
      t[me].c = kid[2];
    } else {
      return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: an unknown node in the expression of %s", op_name);
    }
    node = me;
    return ORCGPU_OK;
  }

  // the class a column takes part as: a Date column is int64 days under a predicate and below a date part, and nothing an
  // expression takes elsewhere
  int col_class(uint32_t col, bool in_date = false) const {
    const int k = agg_class(cols[col].orc_type);
    return (predicate || in_date) && k == ACLASS_DATE ? ACLASS_INT : k;
  }

  // the class of the expression off its leaves (all of `t`: both sides of a predicate's leaf), or the refusal
  int classify() {
    const char *float_col = nullptr, *exact_col = nullptr;
    bool f64_lit = false, dec_lit = false, dec_col = false;
    const char* date_fn = nullptr;  // the first date part of the expression
    const char* int_div = nullptr;  // the first // or % of the expression
    bool has_div = false;           // a / anywhere: an exact expression is a Decimal one
    for (const Node& n : t) {
      if (n.op == ORCGPU_AGG_EXPR_DATE_PART && !date_fn) date_fn = part_name(n.part);
      if ((n.op == ORCGPU_AGG_EXPR_FLOOR_DIV || n.op == ORCGPU_AGG_EXPR_MOD) && !int_div) int_div = division_name(n.op);
      has_div |= n.op == ORCGPU_AGG_EXPR_DIV;
      if (n.op == ORCGPU_AGG_EXPR_LITERAL) {
        // the operand of a date part is a number of days: an exact integer
        if (n.in_date && n.value_type != ORCGPU_PV_INT64)
          return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: %s in the expression of %s takes days, an integer: a %s literal stands below it", part_name(n.part), op_name,
                      n.value_type == ORCGPU_PV_FLOAT64 ? "FLOAT64" : "DECIMAL128");
        f64_lit |= n.value_type == ORCGPU_PV_FLOAT64;
        dec_lit |= n.value_type == ORCGPU_PV_DECIMAL128;
      }
      if (n.op != ORCGPU_AGG_EXPR_COLUMN) continue;
      const AggExprCol& c = cols[n.col];
      const char* name = names[n.col];
      if (c.dict_out) return fail(ORCGPU_UNSUPPORTED, "aggregate: column '%s' is read as a dictionary column: %s on its keys is not supported", name, op_name);
      const int k = col_class(n.col, n.in_date);
      if (predicate && k != ACLASS_INT && k != ACLASS_FLOAT && k != ACLASS_DEC)
        return fail(ORCGPU_UNSUPPORTED, "aggregate: column '%s' cannot stand in the expression of %s: Boolean, String / Varchar / Char / Binary, Timestamp and nested columns are not supported there", name, op_name);
      if (k == ACLASS_TS && c.ts_wide)
        return fail(ORCGPU_UNSUPPORTED, "aggregate: column '%s' is a Timestamp decoded to Decimal128(38, 9): %s is not supported on it", name, op_name);
      if (k != ACLASS_INT && k != ACLASS_FLOAT && k != ACLASS_DEC) return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: the expression of %s does not take column '%s'", op_name, name);
      const uint32_t want = k == ACLASS_FLOAT ? FKIND_FLOAT : k == ACLASS_DEC ? FKIND_DEC128 : FKIND_INT;
      if (c.fkind != want) return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: column '%s' is not decoded to the type the expression of %s needs", name, op_name);
      if (n.in_date && k != ACLASS_INT)
        return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: %s in the expression of %s takes days, a Byte / Short / Int / Long / Date column: not the %s column '%s'", part_name(n.part), op_name,
                    k == ACLASS_FLOAT ? "Float / Double" : "Decimal", name);
      if (k == ACLASS_FLOAT && !float_col) float_col = name;
      if (k != ACLASS_FLOAT && !exact_col) exact_col = name;
      dec_col |= k == ACLASS_DEC;
    }
    if (!float_col && !exact_col && !predicate) return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: the expression of %s holds no column", op_name);
    if (mixed) return ORCGPU_OK;  // (a tree with conversions: the classes meet per node, in type_node)
    if (!float_col && !exact_col && f64_lit && dec_lit)
      return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: the expression of %s holds a FLOAT64 literal beside a DECIMAL128 literal", op_name);
    if (float_col && exact_col)
      return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: the expression of %s mixes the Float / Double column '%s' with the integer or Decimal column '%s': bring one to the other's class with a cast", op_name, float_col, exact_col);
    if (f64_lit && exact_col)
      return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: the expression of %s holds a FLOAT64 literal beside the integer or Decimal column '%s': bring one to the other's class with a cast", op_name, exact_col);
    if (dec_lit && float_col)
      return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: the expression of %s holds a DECIMAL128 literal beside the Float / Double column '%s': bring one to the other's class with a cast", op_name, float_col);
    cls = float_col || (!exact_col && f64_lit) ? XCLASS_FLOAT : (dec_col || dec_lit || has_div) ? XCLASS_DEC : XCLASS_INT;
    // (reached with a date part of literals alone: one over a column has met the mixing rule above)
    if (cls == XCLASS_FLOAT && date_fn)
      return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: the Float / Double expression of %s holds %s, an integer", op_name, date_fn);
    if (cls == XCLASS_FLOAT && int_div)
      return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: the Float / Double expression of %s over column '%s' holds %s, which takes integers", op_name, float_col ? float_col : "", int_div);
    if (cls == XCLASS_FLOAT)
      for (Node& n : t)
        if (n.op == ORCGPU_AGG_EXPR_LITERAL && n.value_type == ORCGPU_PV_INT64) {
          const long long i = (long long)n.iv;
          const double d = (double)i;
          if (!(d >= -9223372036854775808.0 && d < 9223372036854775808.0 && (long long)d == i))
            return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: an INT64 literal beside column '%s' in the expression of %s is not exact as a double", float_col ? float_col : "", op_name);
          n.fv = d;
        }
    return ORCGPU_OK;
  }

  bool is_lit(int n) const { return t[n].op == ORCGPU_AGG_EXPR_LITERAL; }

  // ---- a tree with conversions (include/orcgpu.h: CONVERSIONS): the class of every node, bottom-up ----
  static const char* cast_hint() { return "bring one to the other's class with a cast"; }
  // the two operands x and y of an operator, of CMP, or the value operands of IF / COALESCE, are of one class `k`: an integer
  // beside a Decimal is promoted (the representation is the same), an INT64 literal beside doubles becomes a double when that is
  // exact, a NULL takes its sibling's class; doubles beside anything else are refused
  int meet(int x, int y, int& k) {
    if (t[x].op == ORCGPU_AGG_EXPR_NULL) t[x].nc = t[y].nc;
    if (t[y].op == ORCGPU_AGG_EXPR_NULL) t[y].nc = t[x].nc;
    for (int pass = 0; pass < 2; pass++) {
      Node &p = t[pass ? y : x], &q = t[pass ? x : y];
      if (q.nc != XCLASS_FLOAT || p.nc != XCLASS_INT || p.op != ORCGPU_AGG_EXPR_LITERAL || p.value_type != ORCGPU_PV_INT64) continue;
      const long long i = (long long)p.iv;
      const double d = (double)i;
      if (p.iv != (agg_i128)i || !(d >= -9223372036854775808.0 && d < 9223372036854775808.0 && (long long)d == i))
        return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: an INT64 literal beside column '%s' in the expression of %s is not exact as a double", first_column, op_name);
      p.fv = d;
      p.nc = XCLASS_FLOAT;
      p.value_type = ORCGPU_PV_FLOAT64;
    }
    if ((t[x].nc == XCLASS_FLOAT) != (t[y].nc == XCLASS_FLOAT))
      return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: the expression of %s over column '%s' mixes a Float / Double operand with an integer or Decimal one: %s", op_name, first_column, cast_hint());
    k = t[x].nc == XCLASS_FLOAT ? XCLASS_FLOAT : (t[x].nc == XCLASS_DEC || t[y].nc == XCLASS_DEC) ? XCLASS_DEC : XCLASS_INT;
    return ORCGPU_OK;
  }
  // the class of node n over its typed children, and whether its operands are doubles
  int node_class(int n, int a, int b, int c) {
    const uint32_t op = t[n].op;
    int k = XCLASS_INT;
    if (op == ORCGPU_AGG_EXPR_ADD || op == ORCGPU_AGG_EXPR_SUB || op == ORCGPU_AGG_EXPR_MUL || is_division(op) || op == ORCGPU_AGG_EXPR_CMP || op == ORCGPU_AGG_EXPR_COALESCE) {
      if (const int rc = meet(a, b, k)) return rc;
    } else if (op == ORCGPU_AGG_EXPR_IF) {
      if (const int rc = meet(b, c, k)) return rc;
    } else if (op == ORCGPU_AGG_EXPR_NEG || op == ORCGPU_AGG_EXPR_ABS || op == kScale) {
      k = t[a].nc;
    } else if (op == ORCGPU_AGG_EXPR_DATE_PART) {
      if (t[a].nc == XCLASS_FLOAT)
        return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: %s in the expression of %s over column '%s' takes days, an integer: its operand is a Float / Double (cast it to int64)", part_name(t[n].part), op_name, first_column);
    }
    if ((op == ORCGPU_AGG_EXPR_FLOOR_DIV || op == ORCGPU_AGG_EXPR_MOD) && k == XCLASS_FLOAT)
      return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: %s in the expression of %s over column '%s' takes integers: its operands are Float / Double (cast them to int64)", division_name(op), op_name, first_column);
    t[n].fop = k == XCLASS_FLOAT;
    t[n].nc = is_condition(op) || op == ORCGPU_AGG_EXPR_DATE_PART ? XCLASS_INT : op == ORCGPU_AGG_EXPR_DIV && k == XCLASS_INT ? XCLASS_DEC : k;
    return ORCGPU_OK;
  }
  void set_pow(Node& x, uint32_t k) {
    x.k = k;
    x.iv = agg_pow10(k);
  }
  // A conversion node over its typed child `a`: what it becomes -- the child itself where nothing happens, a literal where the
  // child is one and the conversion does not overflow, else one of the nodes kToF64 .. kF64Round
  int type_conversion(int n, int a, int& out) {
    const uint32_t op = t[n].op;
    const Node ch = t[a];
    const bool f = ch.nc == XCLASS_FLOAT, lit = is_lit(a);
    Node x = t[n];
    x.a = a;
    x.label = ch.label;  // (unary: the slots its operand needs)
    Node folded = ch;    // a literal child's successor
    bool fold = false;
    out = n;
    if (op == ORCGPU_AGG_EXPR_CAST && x.to == XCLASS_FLOAT) {
      if (f) return out = a, ORCGPU_OK;
      x.op = kToF64;
      set_pow(x, (uint32_t)ch.scale);
      x.nc = XCLASS_FLOAT;
      x.scale = 0;
      fold = lit;
      folded.fv = agg_to_f64(ch.iv, x.k, x.iv);
      folded.value_type = ORCGPU_PV_FLOAT64;
    } else if (op == ORCGPU_AGG_EXPR_CAST && x.to == XCLASS_DEC) {
      const int ts = x.want_scale;
      if (f) {
        x.op = kF64ToDec;
        set_pow(x, (uint32_t)ts);
        fold = lit && agg_f64_to_dec(ch.fv, x.iv, &folded.iv);
        folded.value_type = ORCGPU_PV_INT64;
      } else if (ts >= ch.scale) {
        if (ts == ch.scale && !lit && ch.nc != XCLASS_DEC) {
          // an integer to decimal(0): nothing to multiply by, but the CLASS changes -- carried by this node, a "times 10^0" that emits
          // no op, so that the child (a column leaf, say) keeps the class it has
          x.op = kScale;
          set_pow(x, 0);
          x.nc = XCLASS_DEC;
          x.scale = ts;
          t[n] = x;
          return ORCGPU_OK;
        }
        out = scaled(a, (uint32_t)(ts - ch.scale));  // (the child itself where the scales agree: a Decimal already, or a literal)
        t[out].nc = XCLASS_DEC;
        return ORCGPU_OK;
      } else {
        x.op = kRescale;
        x.part = AGG_ROUND_HALF_AWAY;
        set_pow(x, (uint32_t)(ch.scale - ts));
        fold = lit;
        folded.iv = agg_rescale(ch.iv, x.iv, AGG_ROUND_HALF_AWAY);
      }
      x.nc = XCLASS_DEC;
      x.scale = ts;
    } else if (op == ORCGPU_AGG_EXPR_CAST) {  // to int64
      if (f) {
        x.op = kF64ToInt;
        fold = lit && agg_f64_to_i64(ch.fv, &folded.iv);
        folded.value_type = ORCGPU_PV_INT64;
      } else {
        x.op = kToInt;
        set_pow(x, (uint32_t)ch.scale);
        folded.iv = x.k ? agg_rescale(ch.iv, x.iv, AGG_ROUND_TRUNC) : ch.iv;
        fold = lit && folded.iv == (agg_i128)(long long)folded.iv;
      }
      x.nc = XCLASS_INT;
      x.scale = 0;
    } else {  // ROUND, FLOOR, CEIL, TRUNC: the child's class
      const uint32_t mode = op == ORCGPU_AGG_EXPR_ROUND ? AGG_ROUND_HALF_AWAY : op == ORCGPU_AGG_EXPR_FLOOR ? AGG_ROUND_FLOOR : op == ORCGPU_AGG_EXPR_CEIL ? AGG_ROUND_CEIL : AGG_ROUND_TRUNC;
      const int digits = op == ORCGPU_AGG_EXPR_ROUND ? x.want_scale : 0;
      x.nc = ch.nc;
      x.part = mode;
      if (f) {
        if (digits != 0)
          return fail(ORCGPU_UNSUPPORTED, "aggregate: ROUND in the expression of %s over column '%s' rounds a Float / Double to decimal places: only ROUND(x, 0) is a double's; round to n places with a cast to decimal(n)", op_name, first_column);
        x.op = kF64Round;
        fold = lit;
        folded.fv = agg_f64_round(ch.fv, mode);
      } else {
        if (digits >= ch.scale) return out = a, ORCGPU_OK;  // (an integer, or nothing to round away)
        x.op = kRescale;
        set_pow(x, (uint32_t)(ch.scale - digits));
        x.scale = digits;
        fold = lit;
        folded.iv = agg_rescale(ch.iv, x.iv, mode);
      }
    }
    if (fold) {
      folded.nc = x.nc;
      folded.scale = x.scale;
      folded.label = 1;
      t[n] = folded;
    } else {
      t[n] = x;
    }
    return ORCGPU_OK;
  }

  // x <- x * 10^k: folded into a literal when the product fits, else a node of its own (the rows then report the overflow)
  int scaled(int x, uint32_t k) {
    if (!k) return x;
    const agg_i128 f = agg_pow10(k);
    agg_i128 r = 0;
    if (is_lit(x) && agg_mul_checked(t[x].iv, f, &r)) {
      t[x].iv = r;
      t[x].scale += (int)k;
      return x;
    }
    Node n;
    n.op = kScale;
    n.a = x;
    n.k = k;
    n.iv = f;
    n.scale = t[x].scale + (int)k;
    n.nc = t[x].nc;
    n.label = t[x].label;  // (unary: the slots its operand needs)
    t.push_back(n);
    return (int)t.size() - 1;
  }

  // bottom-up: the scales (DEC), the folding of literal-only subtrees, the labels.  Returns the node that stands for `n` now.
  int type_node(int n, int& out) {
    out = n;
    if (t[n].a < 0) return ORCGPU_OK;  // a leaf: label 1, its own scale
    int a = t[n].a, b = t[n].b, c = t[n].c;
    if (const int rc = type_node(a, a)) return rc;
    if (b >= 0)
      if (const int rc = type_node(b, b)) return rc;
    if (c >= 0)
      if (const int rc = type_node(c, c)) return rc;
    const uint32_t op = t[n].op;
    if (mixed) {
      if (is_conversion(op)) return type_conversion(n, a, out);
      if (const int rc = node_class(n, a, b, c)) return rc;
    }
    // (a tree with conversions: an integer is a Decimal of scale 0 wherever its operands are exact, so the scale rule runs there)
    const int kcls = mixed ? (t[n].fop ? XCLASS_FLOAT : t[n].nc) : cls;  // the class the node's folding computes in
    if (mixed ? !t[n].fop : cls == XCLASS_DEC) {
      if (op == ORCGPU_AGG_EXPR_IF || op == ORCGPU_AGG_EXPR_COALESCE) {
        // the two value operands at the larger of their scales; a NULL takes its sibling's
        int &x = op == ORCGPU_AGG_EXPR_IF ? b : a, &y = op == ORCGPU_AGG_EXPR_IF ? c : b;
        if (t[x].op == ORCGPU_AGG_EXPR_NULL) t[x].scale = t[y].scale;
        if (t[y].op == ORCGPU_AGG_EXPR_NULL) t[y].scale = t[x].scale;
        const int s = t[x].scale > t[y].scale ? t[x].scale : t[y].scale;
        if (s <= 38) {
          x = scaled(x, (uint32_t)(s - t[x].scale));
          y = scaled(y, (uint32_t)(s - t[y].scale));
        }
        t[n].scale = s;
      } else if (op == ORCGPU_AGG_EXPR_CMP) {
        const int s = t[a].scale > t[b].scale ? t[a].scale : t[b].scale;
        if (s > 38)
          return fail(ORCGPU_UNSUPPORTED, "aggregate: a node of the expression of %s over column '%s' has a scale of more than 38: it is not supported", op_name, first_column);
        a = scaled(a, (uint32_t)(s - t[a].scale));
        b = scaled(b, (uint32_t)(s - t[b].scale));
        t[n].scale = 0;
      } else if (op == ORCGPU_AGG_EXPR_ABS) {
        t[n].scale = t[a].scale;
      } else if (is_condition(op)) {
        t[n].scale = 0;
      } else if (op == ORCGPU_AGG_EXPR_MUL) {
        t[n].scale = t[a].scale + t[b].scale;
      } else if (op == ORCGPU_AGG_EXPR_DATE_PART) {
        // an integer, over an operand of integers: scale 0 below it too -- but for a division that left another scale there
        if (t[a].scale != 0)
          return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: %s in the expression of %s over column '%s' takes days, an integer: its operand is a quotient of a non-zero scale", part_name(t[n].part), op_name, first_column);
        t[n].scale = 0;
      } else if (op == ORCGPU_AGG_EXPR_DIV) {
        // Q = round(A * 10^k / B) at scale s: the caller's, or min(38, max(6, sa + 4))
        const int sa = t[a].scale, sb = t[b].scale;
        const int s = t[n].want_scale >= 0 ? t[n].want_scale : sa + 4 > 38 ? 38 : sa + 4 < 6 ? 6 : sa + 4;
        const int k = s - sa + sb;
        if (k < 0 || k > 38) {
          snprintf(err, err_len, "aggregate: a division in the expression of %s over column '%s': dividend scale %d, divisor scale %d, result scale %d need the dividend times 10^%d, "
                   "outside 10^0 .. 10^38: not supported", op_name, first_column, sa, sb, s, k);
          return ORCGPU_UNSUPPORTED;
        }
        t[n].scale = s;
        t[n].k = (uint32_t)k;
        t[n].iv = agg_pow10((uint32_t)k);
      } else if (op == ORCGPU_AGG_EXPR_FLOOR_DIV || op == ORCGPU_AGG_EXPR_MOD) {
        if (t[a].scale != 0 || t[b].scale != 0)
          return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: %s in the expression of %s over column '%s' takes integers: an operand has a non-zero scale", division_name(op), op_name, first_column);
        t[n].scale = 0;
      } else if (op == ORCGPU_AGG_EXPR_NEG) {
        t[n].scale = t[a].scale;
      } else {
        const int s = t[a].scale > t[b].scale ? t[a].scale : t[b].scale;
        if (s <= 38) {
          a = scaled(a, (uint32_t)(s - t[a].scale));
          b = scaled(b, (uint32_t)(s - t[b].scale));
        }
        t[n].scale = s;
      }
      if (t[n].scale > 38)
        return fail(ORCGPU_UNSUPPORTED, "aggregate: a node of the expression of %s over column '%s' has a scale of more than 38: it is not supported", op_name, first_column);
    }
    t[n].a = a;
    t[n].b = b;
    t[n].c = c;
    if (is_conditional(op)) {
      if (op == ORCGPU_AGG_EXPR_ABS && is_lit(a)) {  // of a literal: folded with the evaluator's own function unless it overflows
        Node lit = t[a];
        bool ok = true;
        if (kcls == XCLASS_FLOAT) lit.fv = agg_f64_of_bits(agg_bits_of_f64(lit.fv) & 0x7fffffffffffffffull);
        else if (lit.iv < 0) ok = agg_neg_checked(t[a].iv, &lit.iv);
        if (ok) {
          t[n] = lit;
          return ORCGPU_OK;
        }
      }
      // the slots: Sethi-Ullman, and for the ternary node its extension with the condition first -- its result waits in one slot
      // while the two branches are evaluated as a binary node's operands are, the one that needs more first
      const uint32_t la = t[a].label, lb = b >= 0 ? t[b].label : 0, lc = c >= 0 ? t[c].label : 0;
      if (c >= 0) {
        const uint32_t both = lb == lc ? lb + 1 : lb > lc ? lb : lc;
        t[n].label = la > both + 1 ? la : both + 1;
      } else {
        t[n].label = b < 0 ? la : la == lb ? la + 1 : la > lb ? la : lb;
      }
      return ORCGPU_OK;
    }
    if (op == ORCGPU_AGG_EXPR_DATE_PART) {  // of a literal: folded with the evaluator's own function unless it overflows -- then the rows report it
      if (is_lit(a) && t[a].iv == (agg_i128)(int32_t)(long long)t[a].iv) {
        Node lit;
        lit.op = ORCGPU_AGG_EXPR_LITERAL;
        lit.value_type = ORCGPU_PV_INT64;
        lit.iv = agg_date_part((int32_t)(long long)t[a].iv, t[n].part);
        t[n] = lit;
        return ORCGPU_OK;
      }
      t[n].label = t[a].label;  // (unary: the slots its operand needs)
      return ORCGPU_OK;
    }
    if (is_lit(a) && (b < 0 || is_lit(b))) {  // literals alone: folded when the exact result fits
      bool ok = true;
      Node lit;
      lit.op = ORCGPU_AGG_EXPR_LITERAL;
      lit.scale = t[n].scale;
      lit.nc = t[n].nc;
      if (kcls == XCLASS_FLOAT) {
        lit.value_type = ORCGPU_PV_FLOAT64;
        const double x = t[a].fv, y = b >= 0 ? t[b].fv : 0.0;
        lit.fv = op == ORCGPU_AGG_EXPR_ADD ? agg_f64_add(x, y) : op == ORCGPU_AGG_EXPR_SUB ? agg_f64_add(x, -y) : op == ORCGPU_AGG_EXPR_MUL ? agg_f64_mul(x, y)
               : op == ORCGPU_AGG_EXPR_DIV ? agg_f64_div(x, y) : -x;
      } else {
        lit.value_type = ORCGPU_PV_INT64;
        const agg_i128 x = t[a].iv, y = b >= 0 ? t[b].iv : 0;
        ok = op == ORCGPU_AGG_EXPR_ADD ? agg_add_checked(x, y, &lit.iv) : op == ORCGPU_AGG_EXPR_SUB ? agg_sub_checked(x, y, &lit.iv)
           : op == ORCGPU_AGG_EXPR_MUL ? agg_mul_checked(x, y, &lit.iv) : op == ORCGPU_AGG_EXPR_DIV ? agg_div_scaled_checked(x, t[n].iv, y, &lit.iv)
           : op == ORCGPU_AGG_EXPR_FLOOR_DIV ? agg_div_checked(x, y, AGG_DIV_FLOOR, &lit.iv) : op == ORCGPU_AGG_EXPR_MOD ? agg_div_checked(x, y, AGG_DIV_MOD, &lit.iv)
           : agg_neg_checked(x, &lit.iv);
      }
      if (ok) {
        t[n] = lit;
        return ORCGPU_OK;
      }
    }
    const uint32_t la = t[a].label, lb = b >= 0 ? t[b].label : 0;
    t[n].label = b < 0 ? la : la == lb ? la + 1 : la > lb ? la : lb;
    return ORCGPU_OK;
  }

  void emit(int n, std::vector<AggExprOp>& ops) {
    const Node& x = t[n];
    AggExprOp o{};
    if (x.op == ORCGPU_AGG_EXPR_COLUMN) {
      const int k = col_class(x.col, x.in_date);
      o.op = k == ACLASS_FLOAT ? AX_PUSH_F64 : k == ACLASS_DEC ? AX_PUSH_DEC : AX_PUSH_INT;
      o.col = x.col;
      o.lo = cond_program ? 1 : 0;  // (nullable: no gate stands in front of a program with conditionals)
    } else if (x.op == ORCGPU_AGG_EXPR_NULL) {
      o.op = AX_PUSH_NULL;
    } else if (x.op == ORCGPU_AGG_EXPR_ABS || x.op == ORCGPU_AGG_EXPR_IS_NULL || x.op == ORCGPU_AGG_EXPR_NOT) {
      emit(x.a, ops);
      o.op = x.op == ORCGPU_AGG_EXPR_ABS ? AX_ABS : x.op == ORCGPU_AGG_EXPR_IS_NULL ? AX_IS_NULL : AX_NOT;
    } else if (x.op == ORCGPU_AGG_EXPR_IF) {
      // the condition first: it ends in slot 2; then the branch that needs more slots
      const bool else_first = t[x.c].label > t[x.b].label;
      emit(x.a, ops);
      emit(else_first ? x.c : x.b, ops);
      emit(else_first ? x.b : x.c, ops);
      o.op = AX_IF;
      o.col = else_first ? kAggIfElseFirst : kAggIfThenFirst;
    } else if (x.op == ORCGPU_AGG_EXPR_COALESCE || is_condition(x.op)) {  // (CMP, AND, OR: the unary conditions went above)
      const bool right_first = t[x.b].label > t[x.a].label;
      emit(right_first ? x.b : x.a, ops);
      emit(right_first ? x.a : x.b, ops);
      // AND and OR are symmetric; for the other two, a back below b
      if (right_first && (x.op == ORCGPU_AGG_EXPR_COALESCE || x.op == ORCGPU_AGG_EXPR_CMP)) {
        AggExprOp w{};
        w.op = AX_SWAP;
        ops.push_back(w);
      }
      o.op = x.op == ORCGPU_AGG_EXPR_COALESCE ? AX_COALESCE : x.op == ORCGPU_AGG_EXPR_CMP ? AX_CMP : x.op == ORCGPU_AGG_EXPR_AND ? AX_AND : AX_OR;
      if (x.op == ORCGPU_AGG_EXPR_CMP) o.col = x.cmp;
    } else if (x.op == ORCGPU_AGG_EXPR_LITERAL) {
      o.op = AX_PUSH_LIT;
      if ((mixed ? x.nc : cls) == XCLASS_FLOAT) {
        o.lo = agg_bits_of_f64(x.fv);
      } else {
        o.lo = (unsigned long long)x.iv;
        o.hi = (unsigned long long)((agg_u128)x.iv >> 64);
      }
    } else if (x.op == kScale) {
      emit(x.a, ops);
      if (!x.k) return;  // (a cast of an integer to decimal(0): the class alone changed -- type_conversion)
      o.op = AX_SCALE10;
      o.col = x.k;
      o.lo = (unsigned long long)x.iv;
      o.hi = (unsigned long long)((agg_u128)x.iv >> 64);
    } else if (x.op >= kToF64 && x.op <= kF64Round) {  // what the conversion nodes became (type_conversion)
      emit(x.a, ops);
      o.col = x.k;
      o.lo = (unsigned long long)x.iv;
      o.hi = (unsigned long long)((agg_u128)x.iv >> 64);
      if (x.op == kToInt) {
        if (x.k) {
          o.op = AX_RESCALE;
          o.col = x.k | ((uint32_t)AGG_ROUND_TRUNC << 8);
          ops.push_back(o);
        }
        o = AggExprOp{};
        o.op = AX_FIT_I64;
      } else if (x.op == kRescale) {
        o.op = AX_RESCALE;
        o.col = x.k | (x.part << 8);
      } else if (x.op == kF64Round || x.op == kF64ToInt) {
        o = AggExprOp{};
        o.op = x.op == kF64Round ? AX_F64_ROUND : AX_F64_TO_INT;
        o.col = x.op == kF64Round ? x.part : 0;
      } else {
        o.op = x.op == kToF64 ? AX_TO_F64 : AX_F64_TO_DEC;
      }
    } else if (x.op == ORCGPU_AGG_EXPR_NEG) {
      emit(x.a, ops);
      o.op = AX_NEG;
    } else if (x.op == ORCGPU_AGG_EXPR_DATE_PART) {
      emit(x.a, ops);
      o.op = AX_DATE_PART;
      o.col = x.part;
    } else {
      const bool right_first = t[x.b].label > t[x.a].label;
      emit(right_first ? x.b : x.a, ops);
      emit(right_first ? x.a : x.b, ops);
      if (is_division(x.op)) {
        if (right_first) {  // a back below b
          AggExprOp w{};
          w.op = AX_SWAP;
          ops.push_back(w);
        }
        o.op = x.op == ORCGPU_AGG_EXPR_DIV ? AX_DIV : x.op == ORCGPU_AGG_EXPR_FLOOR_DIV ? AX_FLOOR_DIV : AX_MOD;
        if (x.op == ORCGPU_AGG_EXPR_DIV && !(mixed ? x.fop : cls == XCLASS_FLOAT)) {
          o.col = x.k;
          o.lo = (unsigned long long)x.iv;
          o.hi = (unsigned long long)((agg_u128)x.iv >> 64);
        }
      } else {
        o.op = x.op == ORCGPU_AGG_EXPR_ADD ? AX_ADD : x.op == ORCGPU_AGG_EXPR_MUL ? AX_MUL : right_first ? AX_RSUB : AX_SUB;
      }
    }
    // (a program with conversions: the ops that work on either kind say which -- agg_program.h: kAggOpF64)
    if (mixed && x.fop && ((o.op >= AX_ADD && o.op <= AX_NEG) || o.op == AX_DIV || o.op == AX_ABS || o.op == AX_CMP)) o.hi |= kAggOpF64;
    ops.push_back(o);
  }

  bool cond_program = false;  // finish / emit: the program at hand holds a conditional op
  bool holds_conditional(int n) const {
    if (n < 0) return false;
    return is_conditional(t[n].op) || holds_conditional(t[n].a) || holds_conditional(t[n].b) || holds_conditional(t[n].c);
  }

  // pre-order nodes -> a tree behind what `t` holds; root: its root
  int parse_expr(const orcgpu_agg_expr* e, int& root) {
    if (!e || !e->nodes || !e->n_nodes) return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: %s without an expression", op_name);
    if (e->n_nodes > ORCGPU_AGG_EXPR_MAX_NODES) return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: the expression of %s has more than ORCGPU_AGG_EXPR_MAX_NODES (32) nodes", op_name);
    src = e->nodes;
    n_src = e->n_nodes;
    at = 0;
    bool bad_decimal = false;
    {
      const int rc = parse(root);
      if (rc == -1) bad_decimal = true;
      else if (rc) return rc;
    }
    if (bad_decimal) {  // (the column to name may stand behind the literal)
      for (uint32_t k = 0; k < n_src && !*first_column; k++)
        if (src[k].op == ORCGPU_AGG_EXPR_COLUMN && src[k].column) first_column = src[k].column;
      return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: a DECIMAL128 literal of the expression of %s over column '%s' is not 16 bytes of |value| < 10^38 at a scale of 0 .. 38", op_name, first_column);
    }
    if (at != n_src) return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: the expression of %s has nodes left over behind its tree", op_name);
    return check_kinds(root, false, false);
  }
  // Numbers where numbers are wanted, conditions where conditions are: the root is a number, the first child of IF and the children
  // of AND / OR / NOT are conditions, every other operand a number.  null_ok: a NULL node may stand here -- a value operand of IF or
  // COALESCE whose sibling is not a NULL itself.
  int check_kinds(int n, bool want_cond, bool null_ok) {
    const uint32_t op = t[n].op;
    if (is_condition(op) != want_cond)
      return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: %s in the expression of %s over column '%s' stands where a %s is wanted", node_name(op), op_name, first_column,
                  want_cond ? "condition is wanted: it is a number" : "number is wanted: it is a condition");
    if (op == ORCGPU_AGG_EXPR_NULL && !null_ok)
      return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: NULL in the expression of %s over column '%s' stands outside the value operands of IF and COALESCE, or beside another NULL", op_name, first_column);
    const bool kids_cond = op == ORCGPU_AGG_EXPR_AND || op == ORCGPU_AGG_EXPR_OR || op == ORCGPU_AGG_EXPR_NOT;
    const int kid[3] = {t[n].a, t[n].b, t[n].c};
    for (int k = 0; k < 3; k++) {
      if (kid[k] < 0) continue;
      bool cond = kids_cond, nul = false;
      if (op == ORCGPU_AGG_EXPR_IF) {
        cond = k == 0;
        nul = k != 0 && t[kid[k == 1 ? 2 : 1]].op != ORCGPU_AGG_EXPR_NULL;
      } else if (op == ORCGPU_AGG_EXPR_COALESCE) {
        nul = t[kid[1 - k]].op != ORCGPU_AGG_EXPR_NULL;
      }
      if (const int rc = check_kinds(kid[k], cond, nul)) return rc;
    }
    return ORCGPU_OK;
  }
  // the class of everything parsed, and the columns' scales
  int type_leaves() {
    if (const int rc = classify()) return rc;
    if (cls == XCLASS_DEC || mixed)
      for (Node& n : t)
        if (n.op == ORCGPU_AGG_EXPR_COLUMN) n.scale = agg_class(cols[n.col].orc_type) == ACLASS_DEC ? (int)cols[n.col].scale : 0;
    if (mixed)
      for (Node& n : t) {
        if (n.op == ORCGPU_AGG_EXPR_COLUMN) {
          const int k = col_class(n.col, n.in_date);
          n.nc = k == ACLASS_FLOAT ? XCLASS_FLOAT : k == ACLASS_DEC ? XCLASS_DEC : XCLASS_INT;
        } else if (n.op == ORCGPU_AGG_EXPR_LITERAL) {
          n.nc = n.value_type == ORCGPU_PV_FLOAT64 ? XCLASS_FLOAT : n.value_type == ORCGPU_PV_DECIMAL128 ? XCLASS_DEC : XCLASS_INT;
        }
      }
    return ORCGPU_OK;
  }
  // The tree at `root`, parsed from e and typed at its leaves -> its program behind `ops`: scales, folding, labels, the gates,
  // the ops.  root: the node that stands for it afterwards
  int finish(const orcgpu_agg_expr* e, int& root, std::vector<AggExprOp>& ops, bool typed = false) {
    src = e->nodes;
    n_src = e->n_nodes;
    if (!typed)
      if (const int rc = type_node(root, root)) return rc;
    if (t[root].label > kAggExprSlots)
      return fail(ORCGPU_UNSUPPORTED, "aggregate: the expression of %s over column '%s' needs more than ORCGPU_AGG_EXPR_MAX_DEPTH (4) operand slots", op_name, first_column);
    // A tree that still holds a conditional node has no gates: NULL is per operand there, the pushes are nullable and the root's
    // bits decide the row.  Every other program is what it always was.
    // A tree with conversions is laid out the same way, for the mixed interpreter, whether a conditional is left in it or not.
    cond_program = holds_conditional(root) || mixed;
    // the gates: every distinct column, in order of appearance
    std::vector<uint32_t> seen;
    for (uint32_t k = 0; k < n_src && !cond_program; k++) {
      if (src[k].op != ORCGPU_AGG_EXPR_COLUMN) continue;
      uint32_t col = 0;
      while (!names[col] || strcmp(names[col], src[k].column) != 0) col++;  // (parse found it)
      bool dup = false;
      for (uint32_t s : seen) dup |= s == col;
      if (dup) continue;
      seen.push_back(col);
      AggExprOp g{};
      g.op = AX_GATE;
      g.col = col;
      ops.push_back(g);
    }
    const size_t first_op = ops.size();
    if (cond_program) {  // the mark: an interpreter without the conditionals overflows the row on it (agg_program.h: kAggCondMark)
      AggExprOp mark{};
      mark.op = kAggCondMark;
      mark.col = mixed ? kAggConvMarkCol : 0;
      ops.push_back(mark);
    }
    emit(root, ops);
    const size_t end_op = ops.size();  // (what is counted below: not the mark, not the tail)
    if (mixed) {  // the tail that keeps a program with conversions safe in every other interpreter (agg_program.h: kAggConvTail)
      AggExprOp lit{}, mod{}, swap{}, coal{}, add{};
      lit.op = AX_PUSH_LIT;
      mod.op = AX_MOD;
      swap.op = AX_SWAP;
      coal.op = AX_COALESCE;
      add.op = AX_ADD;
      if (cls == XCLASS_FLOAT) {
        lit.lo = kAggCondNaNBits;
        for (const AggExprOp& o : {lit, swap, coal, lit, add}) ops.push_back(o);
      } else {
        for (const AggExprOp& o : {lit, lit, mod, swap, coal}) ops.push_back(o);
      }
    } else if (cond_program && cls == XCLASS_FLOAT) {  // ... and in the double class NaN is its result there: `push NaN, add` behind the program
      AggExprOp nan{}, add{};
      nan.op = AX_PUSH_LIT;
      nan.lo = kAggCondNaNBits;
      add.op = AX_ADD;
      ops.push_back(nan);
      ops.push_back(add);
    }
    // (the labels promise it; the program itself is what the kernels run, so it is counted once more before it is accepted)
    uint32_t depth = 0, most = 0;
    for (size_t k = first_op + (cond_program ? 1 : 0); k < end_op; k++) {
      const uint32_t o = ops[k].op;
      if ((o >= AX_PUSH_INT && o <= AX_PUSH_LIT) || o == AX_PUSH_NULL) depth++;
      else if ((o >= AX_ADD && o <= AX_MUL) || (o >= AX_DIV && o <= AX_MOD)) depth--;  // (AX_NEG, AX_SCALE10, AX_DATE_PART: unary, the depth stays)
      else if (o == AX_SWAP && depth < 2) most = kAggExprSlots + 1;                     // (... and AX_SWAP changes two operands that must be there)
      else if (o == AX_CMP || o == AX_AND || o == AX_OR || o == AX_COALESCE) depth--;   // (AX_IS_NULL, AX_NOT, AX_ABS: unary)
      else if (o == AX_IF && (depth < 3 || ops[k].col > kAggIfElseFirst)) most = kAggExprSlots + 1;
      else if (o == AX_IF) depth -= 2;
      most = depth > most ? depth : most;
    }
    if (most > kAggExprSlots || depth != 1) {
      ops.resize(first_op);
      return fail(ORCGPU_UNSUPPORTED, "aggregate: the expression of %s over column '%s' needs more than ORCGPU_AGG_EXPR_MAX_DEPTH (4) operand slots", op_name, first_column);
    }
    return ORCGPU_OK;
  }

  // The program of `e` goes behind `ops`; kind / scale: the AK_EXPR_* kind and the root's scale (DEC)
  int compile(const orcgpu_agg_expr* e, std::vector<AggExprOp>& ops, uint32_t& kind, int32_t& scale) {
    t.clear();
    mixed = false;
    int root = -1;
    if (const int rc = parse_expr(e, root)) return rc;
    if (const int rc = type_leaves()) return rc;
    if (mixed) {  // the root's class is the expression's
      src = e->nodes;
      n_src = e->n_nodes;
      if (const int rc = type_node(root, root)) return rc;
      cls = t[root].nc;
    }
    if (const int rc = finish(e, root, ops, mixed)) return rc;
    kind = cls == XCLASS_FLOAT ? AK_EXPR_F64 : cls == XCLASS_DEC ? AK_EXPR_DEC : AK_EXPR_INT;
    scale = cls == XCLASS_DEC ? t[root].scale : 0;
    return ORCGPU_OK;
  }

  // One side of a predicate's leaf, compiled: its program, and what its root has become -- a literal (the side held literals
  // alone, or folded to one), a bare column, or neither
  struct Side {
    std::vector<AggExprOp> ops;
    int scale = 0;  // DEC
    bool is_lit = false, is_col = false;
    agg_i128 iv = 0;  // is_lit, INT / DEC
    double fv = 0.0;  // is_lit, FLOAT
    uint32_t col = 0;  // is_col
  };
  // lhs OP rhs: both sides parsed, typed TOGETHER (`cls` is the leaf's), then each finished on its own
  int compile_pair(const orcgpu_agg_expr* lhs, const orcgpu_agg_expr* rhs, Side& l, Side& r) {
    t.clear();
    mixed = false;
    int rl = -1, rr = -1;
    if (const int rc = parse_expr(lhs, rl)) return rc;
    if (const int rc = parse_expr(rhs, rr)) return rc;
    if (const int rc = type_leaves()) return rc;
    if (mixed) {  // the two sides meet as the operands of a comparison do: the leaf's class is theirs
      if (const int rc = type_node(rl, rl)) return rc;
      if (const int rc = type_node(rr, rr)) return rc;
      if (const int rc = meet(rl, rr, cls)) return rc;
    }
    const orcgpu_agg_expr* es[2] = {lhs, rhs};
    int roots[2] = {rl, rr};
    Side* sides[2] = {&l, &r};
    for (int k = 0; k < 2; k++) {
      Side& s = *sides[k];
      s = Side{};
      if (const int rc = finish(es[k], roots[k], s.ops, mixed)) return rc;
      const Node& n = t[roots[k]];
      s.scale = cls == XCLASS_DEC ? n.scale : 0;
      s.is_lit = n.op == ORCGPU_AGG_EXPR_LITERAL;
      s.is_col = n.op == ORCGPU_AGG_EXPR_COLUMN;
      s.iv = n.iv;
      s.fv = n.fv;
      s.col = n.col;
    }
    return ORCGPU_OK;
  }
};

}  // namespace orcgpu_host
