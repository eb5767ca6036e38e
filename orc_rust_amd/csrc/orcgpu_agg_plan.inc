// orcgpu_agg_plan.inc -- the aggregation's plan compiler and its arithmetic on the host, free of HIP
// (tests/hostcheck/agg_plan_check.cpp compiles this very text under AddressSanitizer + UBSan): a list of orcgpu_agg_spec against
// the columns of a result -> the instructions agg_partial_kernel runs (device/agg_program.h), with every refusal of
// orcgpu_result_aggregate (include/orcgpu.h) decided here; the merge of two partial records, which is what the kernels do and what
// the file reader does with its stripes' records; and the last step, a record -> the orcgpu_agg_value handed out, with the range
// checks.  Included behind orcgpu_filter_host.inc, whose FilterColDesc and filter_col_kind say what a decoded column is.
// An aggregate's condition (orcgpu_agg_filter: agg(x) FILTER (WHERE ...)) is a predicate in the row filter's language and is
// compiled by the row filter's compiler (orcgpu_filter_plan.inc) against the same columns: agg_compile_conds, tested by
// tests/hostcheck/agg_filter_plan_check.cpp.
#include <cstdio>
#include <cstring>
#include <vector>

#include "device/agg_program.h"

namespace orcgpu_host {

static_assert(sizeof(AggInsn) == 32 && sizeof(AggPartial) == 48, "agg_program.h: the records the kernels read and write");

// What the plan reads of a column of the result
struct AggCol {
  FilterColDesc d;
  uint32_t scale = 0;   // Decimal
  bool nested = false;  // Struct / List / Map / Union, or a column below one
};

struct AggPlan {
  std::vector<AggInsn> insns;
  std::vector<AggExprOp> ops;  // the programs of the AK_EXPR_* instructions, one behind the other (insn.col: first op, insn.col2: ops)
  // the DISTINCT conditions of the list: their programs one behind the other in one plan (filter_plan_append), and where each
  // lies; insn.cond = k + 1 names cond_spans[k], whose plane agg_cond_eval_kernel fills
  FilterPlan conds;
  std::vector<AggCondSpan> cond_spans;
  char err[256] = {0};
};

// (ACLASS_* / agg_class: orcgpu_agg_expr.inc, which the row filter's plan compiler has included already)
// a column as the expression compiler reads it
inline AggExprCol agg_expr_col(const AggCol& c) {
  AggExprCol x;
  x.orc_type = c.d.orc_type;
  x.scale = c.scale;
  x.fkind = filter_col_kind(c.d);
  x.dict_out = c.d.dict_out;
  x.ts_wide = agg_class(c.d.orc_type) == ACLASS_TS && (c.d.ts_unit > 3 || c.d.width != 8);
  return x;
}
inline const char* agg_op_name(uint32_t op) {
  static const char* const n[] = {"COUNT_ROWS", "COUNT", "SUM", "MIN", "MAX", "SUM_PRODUCT", "SUM_EXPR", "AVG", "AVG_EXPR"};
  return op <= ORCGPU_AGG_OP_AVG_EXPR ? n[op] : "?";
}
inline bool agg_op_is_avg(uint32_t op) { return op == ORCGPU_AGG_OP_AVG || op == ORCGPU_AGG_OP_AVG_EXPR; }

}  // namespace orcgpu_host
#include "orcgpu_agg_expr.inc"
namespace orcgpu_host {

struct AggCompiler {
  const char* const* names;
  const AggCol* cols;
  uint32_t n_columns;
  AggPlan& out;

  int fail(int rc, const char* fmt, const char* a = "", const char* b = "", const char* c = "") {
    snprintf(out.err, sizeof(out.err), fmt, a, b, c);
    return rc;
  }
  int column(const char* name, uint32_t op, uint32_t& col) {
    if (!name) return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: %s without a column name", agg_op_name(op));
    for (uint32_t k = 0; k < n_columns; k++)
      if (names[k] && strcmp(names[k], name) == 0) {
        col = k;
        return ORCGPU_OK;
      }
    return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: column '%s' of %s is not a projected root column", name, agg_op_name(op));
  }
  // the class of a column an op other than COUNT reads the values of, or its refusal
  int value_class(uint32_t op, uint32_t col, int& cls) {
    const AggCol& c = cols[col];
    const char* name = names[col];
    if (c.d.dict_out) return fail(ORCGPU_UNSUPPORTED, "aggregate: column '%s' is read as a dictionary column: %s on its keys is not supported", name, agg_op_name(op));
    cls = agg_class(c.d.orc_type);
    if (cls == ACLASS_TS && (c.d.ts_unit > 3 || c.d.width != 8))
      return fail(ORCGPU_UNSUPPORTED, "aggregate: column '%s' is a Timestamp decoded to Decimal128(38, 9): %s is not supported on it", name, agg_op_name(op));
    const bool sum = op == ORCGPU_AGG_OP_SUM || op == ORCGPU_AGG_OP_SUM_PRODUCT || op == ORCGPU_AGG_OP_AVG;
    if (cls == ACLASS_OTHER || (sum && cls != ACLASS_INT && cls != ACLASS_FLOAT && cls != ACLASS_DEC))
      return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: %s does not take column '%s'", agg_op_name(op), name);
    // ... and what the decode made of it must be what the kernel loads
    const uint32_t want = cls == ACLASS_BOOL ? FKIND_BOOL : cls == ACLASS_FLOAT ? FKIND_FLOAT : cls == ACLASS_DEC ? FKIND_DEC128 : FKIND_INT;
    if (filter_col_kind(c.d) != want) return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: column '%s' is not decoded to the type %s needs", name, agg_op_name(op));
    return ORCGPU_OK;
  }
  // exprs: parallel to specs, or null when no spec has an expression
  int compile(const orcgpu_agg_spec* specs, const orcgpu_agg_expr* exprs, uint32_t n_specs) {
    if (!specs || !n_specs) return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: no aggregates given");
    if (n_specs > ORCGPU_AGG_MAX) return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: more than ORCGPU_AGG_MAX (64) aggregates");
    for (uint32_t k = 0; k < n_columns; k++)
      if (cols[k].nested)
        return fail(ORCGPU_UNSUPPORTED, "aggregate: the result holds the nested column '%s' (Struct / List / Map / Union are not aggregated)", names[k] ? names[k] : "");
    for (uint32_t s = 0; s < n_specs; s++) {
      const orcgpu_agg_spec& sp = specs[s];
      AggInsn in{};
      in.op = sp.op;
      if (sp.op > ORCGPU_AGG_OP_AVG_EXPR) return fail(ORCGPU_INVALID_ARGUMENT, "aggregate: unknown op in the list%s", "");
      if (sp.op == ORCGPU_AGG_OP_SUM_EXPR || sp.op == ORCGPU_AGG_OP_AVG_EXPR) {
        std::vector<AggExprCol> xcols(n_columns);
        for (uint32_t k = 0; k < n_columns; k++) xcols[k] = agg_expr_col(cols[k]);
        AggExprCompiler x{names, xcols.data(), n_columns, agg_op_name(sp.op), out.err, sizeof(out.err)};
        const size_t first = out.ops.size();
        if (const int rc = x.compile(exprs ? &exprs[s] : nullptr, out.ops, in.kind, in.scale)) return rc;
        in.col = (uint32_t)first;
        in.col2 = (uint32_t)(out.ops.size() - first);
        out.insns.push_back(in);
        continue;
      }
      if (sp.op == ORCGPU_AGG_OP_COUNT_ROWS) {
        in.kind = AK_COUNT_ROWS;
        out.insns.push_back(in);
        continue;
      }
      if (const int rc = column(sp.column, sp.op, in.col)) return rc;
      in.col2 = in.col;
      in.fkind = filter_col_kind(cols[in.col].d);
      if (sp.op == ORCGPU_AGG_OP_COUNT) {
        in.kind = AK_COUNT;
        out.insns.push_back(in);
        continue;
      }
      int cls = 0;
      if (const int rc = value_class(sp.op, in.col, cls)) return rc;
      if (sp.op == ORCGPU_AGG_OP_SUM || sp.op == ORCGPU_AGG_OP_AVG) {
        in.kind = cls == ACLASS_INT ? AK_SUM_INT : cls == ACLASS_FLOAT ? AK_SUM_F64 : AK_SUM_DEC;
        in.scale = cls == ACLASS_DEC ? (int32_t)cols[in.col].scale : 0;
      } else if (sp.op == ORCGPU_AGG_OP_SUM_PRODUCT) {
        if (const int rc = column(sp.column2, sp.op, in.col2)) return rc;
        int cls2 = 0;
        if (const int rc = value_class(sp.op, in.col2, cls2)) return rc;
        if (cls != cls2) return fail(ORCGPU_MISMATCHED_SCHEMA, "aggregate: SUM_PRODUCT of columns '%s' and '%s' of different kinds", names[in.col], names[in.col2]);
        in.kind = cls == ACLASS_INT ? AK_SP_INT : cls == ACLASS_FLOAT ? AK_SP_F64 : AK_SP_DEC;
        if (cls == ACLASS_DEC) {
          in.scale = (int32_t)(cols[in.col].scale + cols[in.col2].scale);
          if (in.scale > 38)
            return fail(ORCGPU_UNSUPPORTED, "aggregate: the scales of columns '%s' and '%s' add to more than 38: their SUM_PRODUCT is not supported", names[in.col], names[in.col2]);
        }
      } else {  // MIN, MAX
        in.is_max = sp.op == ORCGPU_AGG_OP_MAX;
        in.kind = cls == ACLASS_FLOAT ? AK_MINMAX_F64 : cls == ACLASS_DEC ? AK_MINMAX_DEC : AK_MINMAX_INT;
        in.scale = cls == ACLASS_DEC ? (int32_t)cols[in.col].scale : cls == ACLASS_TS ? cols[in.col].d.ts_unit : -1;
      }
      out.insns.push_back(in);
    }
    return ORCGPU_OK;
  }
};

// Are two conditions the same, node for node: op, children, column, literal kind and bytes?
inline bool agg_cond_nodes_equal(const orcgpu_agg_filter& a, const orcgpu_agg_filter& b) {
  if (a.n_nodes != b.n_nodes) return false;
  for (uint32_t k = 0; k < a.n_nodes; k++) {
    const orcgpu_predicate_node &x = a.nodes[k], &y = b.nodes[k];
    if (x.op != y.op || x.n_children != y.n_children || x.value_type != y.value_type || (x.value_is_null != 0) != (y.value_is_null != 0) || x.i != y.i ||
        memcmp(&x.f, &y.f, sizeof(double)) != 0 || x.s_len != y.s_len || !x.column != !y.column || !x.s != !y.s)
      return false;
    if (x.column && strcmp(x.column, y.column) != 0) return false;
    if (x.s && x.s_len && memcmp(x.s, y.s, (size_t)x.s_len) != 0) return false;
  }
  return true;
}

// The conditions of a list, filters[0 .. n) parallel to its specs ({NULL, 0}: the spec has none) -> out.conds / out.cond_spans and
// cond_of[s] = 0 or k + 1 for spec s (n_nodes = 0: none).  Every condition is compiled by filter_compile against the columns the aggregates were
// compiled against -- the row filter's nodes, literal rules, depth limit, statuses and messages --; conditions that are node for
// node the same share one program and one plane; more than ORCGPU_AGG_MAX distinct ones are ORCGPU_INVALID_ARGUMENT.  A condition
// that reads the values of a column read as a dictionary column is ORCGPU_UNSUPPORTED, as under the row filter.
inline int agg_compile_conds(const orcgpu_agg_filter* filters, uint32_t n, const char* const* names, const AggCol* cols, uint32_t n_columns, AggPlan& out,
                             std::vector<uint32_t>& cond_of, const KeySetRefs* sets = nullptr) {
  out.conds = FilterPlan{};
  out.cond_spans.clear();
  cond_of.assign(n, 0);
  if (!filters) return ORCGPU_OK;
  std::vector<int32_t> kinds(n_columns), params(n_columns);
  for (uint32_t c = 0; c < n_columns; c++) {
    kinds[c] = cols[c].d.orc_type;
    params[c] = kinds[c] == ORCGPU_T_DECIMAL ? (int32_t)cols[c].scale : cols[c].d.ts_unit;
  }
  std::vector<uint32_t> first_spec;  // per distinct condition: the spec that brought it
  for (uint32_t s = 0; s < n; s++) {
    const orcgpu_agg_filter& f = filters[s];
    if (!f.n_nodes) continue;  // (no condition, whatever `nodes` holds: what orcgpu_reader_set_aggregate_filters takes it for too)
    if (!f.nodes) {
      snprintf(out.err, sizeof(out.err), "aggregate: the condition of aggregate %u has a node count and no nodes", s);
      return ORCGPU_INVALID_ARGUMENT;
    }
    uint32_t k = 0;
    while (k < first_spec.size() && !agg_cond_nodes_equal(filters[first_spec[k]], f)) k++;
    if (k == first_spec.size()) {
      if (k == ORCGPU_AGG_MAX) {
        snprintf(out.err, sizeof(out.err), "aggregate: more than ORCGPU_AGG_MAX (64) distinct conditions");
        return ORCGPU_INVALID_ARGUMENT;
      }
      FilterPlan one;
      if (const int rc = filter_compile(f.nodes, f.n_nodes, names, kinds.data(), n_columns, one, params.data(), sets)) {
        memcpy(out.err, one.err, sizeof(out.err));
        return rc;
      }
      for (const FilterInsn& in : one.prog) {
        if (fop_reads_values(in.op) && in.col < n_columns && cols[in.col].d.dict_out) {
          filter_dict_refusal(out.err, sizeof(out.err), names[in.col] ? names[in.col] : "", in.col);
          return ORCGPU_UNSUPPORTED;
        }
        if (in.op != FOP_CMP_EXPR) continue;
        std::vector<FilterExprRead> reads;  // (an expression leaf reads the values of several columns)
        filter_expr_reads(one, in, reads);
        for (const FilterExprRead& rd : reads)
          if (rd.col < n_columns && cols[rd.col].d.dict_out) {
            filter_dict_refusal(out.err, sizeof(out.err), names[rd.col] ? names[rd.col] : "", rd.col);
            return ORCGPU_UNSUPPORTED;
          }
      }
      const uint32_t first = filter_plan_append(out.conds, one);
      out.cond_spans.push_back(AggCondSpan{first, (uint32_t)one.prog.size()});
      first_spec.push_back(s);
    }
    cond_of[s] = k + 1;
  }
  return ORCGPU_OK;
}

// filters: parallel to specs like exprs, or null when no spec has a condition
inline int agg_compile(const orcgpu_agg_spec* specs, const orcgpu_agg_expr* exprs, const orcgpu_agg_filter* filters, uint32_t n_specs, const char* const* names,
                       const AggCol* cols, uint32_t n_columns, AggPlan& out, const KeySetRefs* sets = nullptr) {
  out.insns.clear();
  out.ops.clear();
  out.conds = FilterPlan{};
  out.cond_spans.clear();
  out.err[0] = 0;
  AggCompiler c{names, cols, n_columns, out};
  if (const int rc = c.compile(specs, exprs, n_specs)) return rc;
  std::vector<uint32_t> cond_of;  // (one instruction per spec: an AVG is its sum, finished over the count)
  if (const int rc = agg_compile_conds(filters, n_specs, names, cols, n_columns, out, cond_of, sets)) return rc;
  for (uint32_t s = 0; s < n_specs; s++) out.insns[s].cond = cond_of[s];
  return ORCGPU_OK;
}
inline int agg_compile(const orcgpu_agg_spec* specs, const orcgpu_agg_expr* exprs, uint32_t n_specs, const char* const* names, const AggCol* cols, uint32_t n_columns,
                       AggPlan& out) {
  return agg_compile(specs, exprs, nullptr, n_specs, names, cols, n_columns, out);
}

// Do the instructions read what is there?  A column index below nc; a program inside the op table whose every op names a column
// below nc; a condition among the n_conds planes of the call.  (The plan was compiled against these columns: anything else is a
// caller's mix-up, ORCGPU_UNEXPECTED before any launch.)
inline bool agg_plan_in_bounds(const std::vector<AggInsn>& insns, const std::vector<AggExprOp>& ops, uint32_t nc, uint32_t n_conds = 0) {
  for (const AggInsn& in : insns) {
    if (in.cond > n_conds) return false;
    if (in.kind == AK_COUNT_ROWS) continue;
    if (!agg_is_expr(in.kind)) {
      if (in.kind >= AK_N || in.col >= nc || in.col2 >= nc) return false;
      continue;
    }
    if (in.col > ops.size() || in.col2 > ops.size() - in.col || !in.col2) return false;
    for (uint32_t k = in.col; k < in.col + in.col2; k++)
      if (ops[k].op >= AX_N || (ops[k].op <= AX_PUSH_F64 && ops[k].col >= nc) || (ops[k].op == AX_DATE_PART && ops[k].col >= AX_PART_N) || (ops[k].op == AX_DIV && ops[k].col > 38) ||
          (ops[k].op == AX_CMP && ops[k].col > 5) || (ops[k].op == AX_IF && ops[k].col > kAggIfElseFirst)) return false;
  }
  return true;
}
// ... and the conditions' programs: inside the n_insn instructions of the call's predicate program, from `first` on
inline bool agg_conds_in_bounds(const std::vector<AggCondSpan>& spans, uint32_t first, size_t n_insn) {
  for (const AggCondSpan& sp : spans)
    if (!sp.n || (uint64_t)first + sp.first + sp.n > n_insn) return false;
  return true;
}
inline int agg_compile(const orcgpu_agg_spec* specs, uint32_t n_specs, const char* const* names, const AggCol* cols, uint32_t n_columns, AggPlan& out) {
  return agg_compile(specs, nullptr, n_specs, names, cols, n_columns, out);
}

// ---- the arithmetic: signed 192-bit integers as three little-endian words ----
inline void agg_add192(unsigned long long* a, const unsigned long long* b) {
  unsigned long long carry = 0;
  for (int k = 0; k < 3; k++) {
    const unsigned long long t = a[k] + b[k];
    const unsigned long long c1 = t < b[k];
    a[k] = t + carry;
    carry = c1 | (unsigned long long)(a[k] < carry);
  }
}
inline bool agg_less_i128(const unsigned long long* a, const unsigned long long* b) {
  return (long long)a[1] < (long long)b[1] || (a[1] == b[1] && a[0] < b[0]);
}
// does the value fit a signed 128-bit integer?
inline bool agg_fits_i128(const unsigned long long* w) { return w[2] == (unsigned long long)((long long)w[1] >> 63); }
// |value| < 10^38, what a Decimal128 may hold
inline bool agg_fits_decimal(const unsigned long long* w) {
  unsigned long long m[3] = {w[0], w[1], w[2]};
  if ((long long)m[2] < 0) {  // -v = ~v + 1
    unsigned long long one[3] = {1, 0, 0};
    for (auto& x : m) x = ~x;
    agg_add192(m, one);
  }
  const unsigned long long hi = 0x4b3b4ca85a86c47aull, lo = 0x098a224000000000ull;  // 10^38
  return m[2] == 0 && (m[1] < hi || (m[1] == hi && m[0] < lo));
}

// into <- into (+) from: what agg_fold (device/agg_kernels.hip) does, on the host -- the reader's stripes in stripe order
inline void agg_merge(const AggInsn& in, AggPartial& into, const AggPartial& from) {
  into.flags |= from.flags;
  if (agg_is_float_sum(in.kind)) {
    into.f += from.f;
  } else if (agg_is_wide_sum(in.kind)) {
    agg_add192(into.w, from.w);
  } else if (from.count) {
    bool take = !into.count;
    if (!take) {
      if (in.kind == AK_MINMAX_INT) take = in.is_max ? (long long)from.w[0] > (long long)into.w[0] : (long long)from.w[0] < (long long)into.w[0];
      else if (in.kind == AK_MINMAX_DEC) take = in.is_max ? agg_less_i128(into.w, from.w) : agg_less_i128(from.w, into.w);
      else take = in.is_max ? from.f > into.f : from.f < into.f;
    }
    if (take) {
      into.w[0] = from.w[0];
      into.w[1] = from.w[1];
      into.f = from.f;
    }
  }
  into.count += from.count;
}

// The record of an instruction -> what the caller gets
inline void agg_finish(const AggInsn& in, const AggPartial& p, orcgpu_agg_value* v) {
  memset(v, 0, sizeof(*v));
  const bool sticky = (p.flags & AGG_OVERFLOW) != 0;
  if (agg_op_is_avg(in.op)) {  // the exact sum over the count of values, finished here
    v->is_null = p.count == 0;
    if (agg_is_float_sum(in.kind)) {
      v->kind = ORCGPU_AGG_KIND_F64;
      v->f = p.count ? p.f / (double)p.count : 0.0;
      v->overflow = sticky;  // (an expression of doubles alone: a conversion inside it overflowed a row -- include/orcgpu.h: CONVERSIONS)
    } else if (in.kind == AK_SUM_DEC || in.kind == AK_EXPR_DEC) {
      v->kind = ORCGPU_AGG_KIND_DEC128;
      v->scale_or_unit = in.scale + 4 < 38 ? in.scale + 4 : 38;
      v->overflow = !agg_fits_decimal(p.w) || sticky;
      if (p.count && !v->overflow) {
        uint32_t scale = 0;
        unsigned long long q[3];
        agg_avg_decimal(p.w, p.count, (uint32_t)in.scale, &scale, q);
        v->overflow = !agg_fits_decimal(q);
        for (int k = 0; k < 3; k++) v->w[k] = q[k];
      }
    } else {  // AK_SUM_INT, AK_EXPR_INT
      v->kind = ORCGPU_AGG_KIND_F64;
      v->overflow = !agg_fits_i128(p.w) || sticky;
      if (p.count && !v->overflow) v->f = agg_avg_int(agg_i128_of(p.w[0], p.w[1]), p.count);
    }
    return;
  }
  switch (in.kind) {
    case AK_COUNT_ROWS:
    case AK_COUNT:
      v->kind = ORCGPU_AGG_KIND_U64;
      v->w[0] = p.w[0];
      return;
    case AK_SUM_INT:
    case AK_SP_INT:
    case AK_EXPR_INT:
      v->kind = ORCGPU_AGG_KIND_I128;
      v->is_null = p.count == 0;
      v->overflow = !agg_fits_i128(p.w) || sticky;
      break;
    case AK_SUM_DEC:
    case AK_SP_DEC:
    case AK_EXPR_DEC:
      v->kind = ORCGPU_AGG_KIND_DEC128;
      v->scale_or_unit = in.scale;
      v->is_null = p.count == 0;
      v->overflow = !agg_fits_decimal(p.w) || sticky;
      break;
    case AK_SUM_F64:
    case AK_SP_F64:
    case AK_EXPR_F64:
      v->kind = ORCGPU_AGG_KIND_F64;
      v->is_null = p.count == 0;
      v->f = p.f;
      v->overflow = sticky;  // (AK_EXPR_F64 alone sets it: a conversion inside the expression overflowed a row)
      return;
    case AK_MINMAX_INT:
      v->kind = ORCGPU_AGG_KIND_I64;
      v->scale_or_unit = in.scale;
      v->is_null = p.count == 0;
      v->w[0] = p.count ? p.w[0] : 0;
      return;
    case AK_MINMAX_DEC:
      v->kind = ORCGPU_AGG_KIND_DEC128;
      v->scale_or_unit = in.scale;
      v->is_null = p.count == 0;
      if (p.count) {
        v->w[0] = p.w[0];
        v->w[1] = p.w[1];
        v->w[2] = (unsigned long long)((long long)p.w[1] >> 63);
      }
      return;
    default:  // AK_MINMAX_F64: NaN only when every value was one
      v->kind = ORCGPU_AGG_KIND_F64;
      v->is_null = p.count == 0 && !(p.flags & AGG_SAW_NAN);
      v->f = p.count ? p.f : ((p.flags & AGG_SAW_NAN) ? __builtin_nan("") : 0.0);
      return;
  }
  if (!v->is_null)
    for (int k = 0; k < 3; k++) v->w[k] = p.w[k];
}

}  // namespace orcgpu_host
