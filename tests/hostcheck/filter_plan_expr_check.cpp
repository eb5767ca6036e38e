// filter_plan_expr_check -- the row filter's expression leaf (ORCGPU_PRED_CMP_EXPR: lhs OP rhs) through the plan compiler, compiled
// for the HOST under AddressSanitizer + UBSan (tests/test_filter_plan_expr_sanitized.py).  It includes the very text liborcgpu.so is
// built from -- orcgpu_filter_plan.inc, and through it orcgpu_agg_expr.inc, device/agg_expr_eval.h and device/filter_expr_eval.h --
// and does two things with the cases it is given: it prints what became of each leaf (the status, the instruction, its planes),
// and it EVALUATES the compiled leaf on the case's rows with the evaluator and the comparison the kernel runs, printing T / F / U
// (UNKNOWN by a NULL) / O (UNKNOWN by an overflow inside a side) per row.  The test judges both against tests/filter_model_expr.py.
// Then, without a case file: malformed node lists, the plane numbering beside a LIKE and an IN leaf, and filter_plan_append.
//
//   case <name> <cmp 0..5> <n_columns> L <tokens> R <tokens>      tokens, in pre-order: c:<column> i:<int64> f:<hex bits of a double>
//   row <column>=<value> ...                                      d:<unscaled>:<scale> + - * neg;  values: an integer, x<hex bits>, N
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/orcgpu.h"
#include "../../orc_rust_amd/csrc/orcgpu_filter_plan.inc"

using namespace orcgpu_host;

struct Column {
  const char* name;
  int32_t kind, param;
};
static const Column kColumns[] = {
    {"i8", ORCGPU_T_BYTE, 0},      {"i32", ORCGPU_T_INT, 0},     {"i64", ORCGPU_T_LONG, 0},    {"j64", ORCGPU_T_LONG, 0},          {"k64", ORCGPU_T_LONG, 0},
    {"d", ORCGPU_T_DATE, 0},       {"e", ORCGPU_T_DATE, 0},      {"f32", ORCGPU_T_FLOAT, 0},   {"f64", ORCGPU_T_DOUBLE, 0},        {"g64", ORCGPU_T_DOUBLE, 0},
    {"p", ORCGPU_T_DECIMAL, 2},    {"q", ORCGPU_T_DECIMAL, 7},   {"w", ORCGPU_T_DECIMAL, 0},   {"v", ORCGPU_T_DECIMAL, 0},         {"z", ORCGPU_T_DECIMAL, 20},
    {"b", ORCGPU_T_BOOLEAN, 0},    {"s", ORCGPU_T_STRING, 0},    {"vc", ORCGPU_T_VARCHAR, 0},  {"ch", ORCGPU_T_CHAR, 0},           {"bin", ORCGPU_T_BINARY, 0},
    {"ts", ORCGPU_T_TIMESTAMP, 2}, {"tsi", ORCGPU_T_TIMESTAMP_INSTANT, 3},                     {"st", ORCGPU_T_STRUCT, 0}};
constexpr uint32_t kAll = sizeof(kColumns) / sizeof(kColumns[0]), kFlat = kAll - 1;  // (the last one is nested)

static std::vector<const char*> g_names;
static std::vector<int32_t> g_kinds, g_params;

static agg_i128 num(const std::string& s) {
  agg_i128 v = 0;
  size_t k = s[0] == '-';
  for (; k < s.size(); k++) v = v * 10 + (s[k] - '0');
  return s[0] == '-' ? -v : v;
}

struct Holder {
  std::vector<std::unique_ptr<std::string>> strs;
  const char* keep(const std::string& s) {
    strs.emplace_back(new std::string(s));
    return strs.back()->data();
  }
};

static orcgpu_predicate_node enode(int32_t op, uint32_t kids) {
  orcgpu_predicate_node n{};
  n.op = op;
  n.n_children = kids;
  return n;
}
static orcgpu_predicate_node token(const std::string& t, Holder& hold) {
  if (t == "+") return enode(ORCGPU_PRED_EXPR_ADD, 2);
  if (t == "-") return enode(ORCGPU_PRED_EXPR_SUB, 2);
  if (t == "*") return enode(ORCGPU_PRED_EXPR_MUL, 2);
  if (t == "neg") return enode(ORCGPU_PRED_EXPR_NEG, 1);
  orcgpu_predicate_node n = enode(t[0] == 'c' ? ORCGPU_PRED_EXPR_COLUMN : ORCGPU_PRED_EXPR_LITERAL, 0);
  const std::string rest = t.substr(2);
  if (t[0] == 'c') n.column = hold.keep(rest + '\0');
  else if (t[0] == 'i') {
    n.value_type = ORCGPU_PV_INT64;
    n.i = (int64_t)num(rest);
  } else if (t[0] == 'f') {
    n.value_type = ORCGPU_PV_FLOAT64;
    n.f = agg_f64_of_bits(strtoull(rest.c_str(), nullptr, 16));
  } else {
    const size_t colon = rest.find(':');
    const agg_i128 v = num(rest.substr(0, colon));
    n.value_type = ORCGPU_PV_DECIMAL128;
    n.i = atoi(rest.c_str() + colon + 1);
    n.s = hold.keep(std::string(reinterpret_cast<const char*>(&v), 16));
    n.s_len = 16;
  }
  return n;
}
static orcgpu_predicate_node cmp_node(int64_t cmp, uint32_t kids = 2) {
  orcgpu_predicate_node n = enode(ORCGPU_PRED_CMP_EXPR, kids);
  n.i = cmp;
  return n;
}

static int compile(const std::vector<orcgpu_predicate_node>& nodes, uint32_t n_columns, FilterPlan& plan) {
  return filter_compile(nodes.data(), (uint32_t)nodes.size(), g_names.data(), g_kinds.data(), n_columns, plan, g_params.data());
}
static int named(const FilterPlan& plan, const char* column) { return std::string(plan.err).find(std::string("'") + column + "'") != std::string::npos; }

// ---- a row, as agg_expr_eval_* reads it ----
struct HostRow {
  std::map<uint32_t, agg_i128> ints;  // int64 / Date values and Decimal unscaled values
  std::map<uint32_t, double> floats;
  bool valid(uint32_t col) const { return ints.count(col) || floats.count(col); }
  agg_i128 load_int(uint32_t col) const { return ints.at(col); }
  agg_i128 load_dec(uint32_t col) const { return ints.at(col); }
  double load_f64(uint32_t col) const { return floats.at(col); }
};

// the one-instruction programs a leaf may compile to, on a row: what filter_eval_word does for them
static char eval_leaf(const FilterPlan& plan, const HostRow& row) {
  const FilterInsn& in = plan.prog[0];
  if (in.op == FOP_TRUE) return 'T';
  if (in.op == FOP_FALSE) return 'F';
  if (in.op == FOP_CMP_INT || in.op == FOP_CMP_DEC128) {
    if (!row.valid(in.col)) return 'U';
    const agg_i128 v = row.ints.at(in.col), l = in.op == FOP_CMP_INT ? (agg_i128)in.i : agg_i128_of(in.lo, (unsigned long long)in.i);
    return filter_expr_answer(in.cmp, v < l, v == l, v > l) ? 'T' : 'F';
  }
  if (in.op == FOP_CMP_FLOAT) {
    if (!row.valid(in.col)) return 'U';
    return filter_expr_compare_f64(in.cmp, row.floats.at(in.col), in.f) ? 'T' : 'F';
  }
  FilterExprBlob e;
  if (in.op != FOP_CMP_EXPR || !filter_expr_blob(plan.lits.data() + in.lit_off, in.lit_len, &e)) return '?';
  // (the blob lies 8-byte aligned in a byte vector: the ops are read from an aligned copy)
  std::vector<AggExprOp> ops(e.n_lhs + e.n_rhs);
  memcpy(ops.data(), plan.lits.data() + in.lit_off + kExprHeaderBytes, ops.size() * sizeof(AggExprOp));
  int sl, sr;
  bool t;
  if (e.cls == FXC_FLOAT) {
    double a = 0, b = 0;
    sl = agg_expr_eval_f64(ops.data(), e.n_lhs, row, &a);
    sr = agg_expr_eval_f64(ops.data() + e.n_lhs, e.n_rhs, row, &b);
    t = filter_expr_compare_f64(in.cmp, a, b);
  } else {
    agg_i128 a = 0, b = 0;
    sl = agg_expr_eval_i128(ops.data(), e.n_lhs, row, &a);
    sr = agg_expr_eval_i128(ops.data() + e.n_lhs, e.n_rhs, row, &b);
    t = filter_expr_compare_i128(in.cmp, a, b, e.d, e.p10);
  }
  if (sl == AGG_ROW_NULL || sr == AGG_ROW_NULL) return 'U';
  if (sl == AGG_ROW_OVERFLOW || sr == AGG_ROW_OVERFLOW) return 'O';
  return t ? 'T' : 'F';
}

static uint32_t column_index(const std::string& name) {
  for (uint32_t k = 0; k < kAll; k++)
    if (name == kColumns[k].name) return k;
  fprintf(stderr, "no column %s\n", name.c_str());
  exit(2);
}

static void print_insn(const char* tag, const char* name, int rc, const FilterPlan& plan, const char* column) {
  if (rc) {
    printf("%s %s %d %d\n", tag, name, rc, column ? named(plan, column) : 0);
    return;
  }
  const FilterInsn& in = plan.prog[0];
  FilterExprBlob e{};
  const bool blob = in.op == FOP_CMP_EXPR && filter_expr_blob(plan.lits.data() + in.lit_off, in.lit_len, &e);
  printf("%s %s 0 %zu %u %u %lld %llu %llx %u %zu %zu cls=%d d=%d ops=%u,%u aligned=%d\n", tag, name, plan.prog.size(), in.op, in.cmp, in.i, in.lo, agg_bits_of_f64(in.f), in.col,
         plan.expr_leaves.size(), plan.n_planes(), blob ? (int)e.cls : -1, blob ? e.d : 0, blob ? e.n_lhs : 0, blob ? e.n_rhs : 0, (int)((in.lit_off & 7) == 0));
}

int main(int argc, char** argv) {
  for (const Column& c : kColumns) {
    g_names.push_back(c.name);
    g_kinds.push_back(c.kind);
    g_params.push_back(c.param);
  }
  if (argc > 1) {
    std::ifstream f(argv[1]);
    std::string line, name;
    FilterPlan plan;
    int rc = -1;
    uint32_t row_no = 0;
    while (std::getline(f, line)) {
      std::istringstream ss(line);
      std::string what, tok;
      ss >> what;
      if (what == "case") {
        Holder hold;
        int cmp = 0;
        uint32_t n_columns = 0;
        std::string refused;
        ss >> name >> cmp >> n_columns >> refused;  // refused: the column a refusal must name, or -
        std::vector<orcgpu_predicate_node> nodes = {cmp_node(cmp)};
        while (ss >> tok)
          if (tok != "L" && tok != "R") nodes.push_back(token(tok, hold));
        rc = compile(nodes, n_columns ? n_columns : kFlat, plan);
        print_insn("case", name.c_str(), rc, plan, refused == "-" ? nullptr : refused.c_str());
        row_no = 0;
      } else if (what == "row" && rc == 0) {
        HostRow row;
        while (ss >> tok) {
          const size_t eq = tok.find('=');
          const uint32_t col = column_index(tok.substr(0, eq));
          const std::string v = tok.substr(eq + 1);
          if (v == "N") continue;
          if (v[0] == 'x') row.floats[col] = agg_f64_of_bits(strtoull(v.c_str() + 1, nullptr, 16));
          else row.ints[col] = num(v);
        }
        printf("row %s %u %c\n", name.c_str(), row_no++, eval_leaf(plan, row));
      }
    }
  }
  // ---- malformed node lists ----
  Holder hold;
  auto T = [&](const char* t) { return token(t, hold); };
  auto bad = [&](const char* name, const std::vector<orcgpu_predicate_node>& nodes) {
    FilterPlan plan;
    const int rc = compile(nodes, kFlat, plan);
    printf("bad %s %d\n", name, rc);
  };
  bad("expr_column_alone", {T("c:i64")});
  bad("expr_literal_under_and", {enode(ORCGPU_PRED_AND, 1), T("i:1")});
  bad("expr_add_under_not", {enode(ORCGPU_PRED_NOT, 1), T("+"), T("c:i64"), T("i:1")});
  bad("one_side", {cmp_node(ORCGPU_PRED_LT, 1), T("c:i64")});
  bad("three_sides", {cmp_node(ORCGPU_PRED_LT, 3), T("c:i64"), T("i:1"), T("i:2")});
  bad("ends_inside_rhs", {cmp_node(ORCGPU_PRED_LT), T("c:i64"), T("+"), T("i:1")});
  bad("ends_before_rhs", {cmp_node(ORCGPU_PRED_LT), T("c:i64")});
  bad("op_6", {cmp_node(6), T("c:i64"), T("i:1")});
  bad("op_minus_1", {cmp_node(-1), T("c:i64"), T("i:1")});
  bad("add_with_one_child", {cmp_node(ORCGPU_PRED_LT), enode(ORCGPU_PRED_EXPR_ADD, 1), T("c:i64"), T("i:1")});
  bad("column_with_a_child", {cmp_node(ORCGPU_PRED_LT), enode(ORCGPU_PRED_EXPR_COLUMN, 1), T("c:i64"), T("i:1")});
  bad("neg_with_two", {cmp_node(ORCGPU_PRED_LT), enode(ORCGPU_PRED_EXPR_NEG, 2), T("c:i64"), T("i:1"), T("i:1")});
  {
    orcgpu_predicate_node leaf{};  // a comparison leaf inside an expression
    leaf.op = ORCGPU_PRED_LT;
    leaf.column = "i64";
    leaf.value_type = ORCGPU_PV_INT64;
    bad("comparison_inside", {cmp_node(ORCGPU_PRED_LT), leaf, T("i:1")});
    orcgpu_predicate_node null_lit = T("i:1");
    null_lit.value_is_null = 1;
    bad("null_literal", {cmp_node(ORCGPU_PRED_LT), T("c:i64"), null_lit});
    orcgpu_predicate_node nameless = enode(ORCGPU_PRED_EXPR_COLUMN, 0);
    bad("column_without_a_name", {cmp_node(ORCGPU_PRED_LT), nameless, T("i:1")});
    orcgpu_predicate_node bool_lit = T("i:1");
    bool_lit.value_type = ORCGPU_PV_BOOLEAN;
    bad("boolean_literal", {cmp_node(ORCGPU_PRED_LT), T("c:i64"), bool_lit});
  }
  bad("nodes_behind_the_root", {cmp_node(ORCGPU_PRED_LT), T("c:i64"), T("i:1"), T("i:2")});
  bad("no_such_column", {cmp_node(ORCGPU_PRED_LT), T("c:nope"), T("i:1")});
  bad("fine", {cmp_node(ORCGPU_PRED_LT), T("c:i64"), T("c:j64")});
  // the leaf counts toward the depth as a leaf alone: 63 NOTs above it are 64 levels, 64 are one too many
  for (uint32_t nots : {63u, 64u}) {
    std::vector<orcgpu_predicate_node> nodes(nots, enode(ORCGPU_PRED_NOT, 1));
    for (const char* t : {"+", "c:i64", "*", "c:j64", "c:k64"}) {
      if (nodes.size() == nots) nodes.push_back(cmp_node(ORCGPU_PRED_GT));
      nodes.push_back(T(t));
    }
    nodes.push_back(T("i:0"));
    FilterPlan plan;
    const int rc = compile(nodes, kFlat, plan);
    printf("depth %u %d %u\n", nots, rc, plan.depth);
  }

  // ---- plane numbering and leaf lists: a LIKE, an expression leaf, an IN, a folded leaf, another expression leaf ----
  auto strleaf = [&](int op, const char* col, const char* s, uint32_t kids = 0) {
    orcgpu_predicate_node n{};
    n.op = op;
    n.column = col;
    n.n_children = kids;
    n.value_type = ORCGPU_PV_UTF8;
    n.s = s;
    n.s_len = s ? strlen(s) : 0;
    return n;
  };
  auto intlit = [&](int64_t v) {
    orcgpu_predicate_node n{};
    n.op = ORCGPU_PRED_LITERAL;
    n.value_type = ORCGPU_PV_INT64;
    n.i = v;
    return n;
  };
  auto dump = [&](const char* tag, const FilterPlan& plan) {
    printf("%s", tag);
    for (const FilterInsn& in : plan.prog) printf(" %u:%lld:%u:%llu", in.op, in.i, in.cmp, (unsigned long long)(in.lit_off & 7));
    printf(" | like");
    for (uint32_t k : plan.like_leaves) printf(" %u", k);
    printf(" in");
    for (uint32_t k : plan.in_leaves) printf(" %u", k);
    printf(" expr");
    for (uint32_t k : plan.expr_leaves) printf(" %u", k);
    printf(" planes %zu leaves %zu\n", plan.n_planes(), plan.n_leaves());
  };
  std::vector<orcgpu_predicate_node> five = {enode(ORCGPU_PRED_OR, 5),
                                             strleaf(ORCGPU_PRED_LIKE, "s", "a%b"),
                                             cmp_node(ORCGPU_PRED_LT), T("c:d"), T("c:e"),
                                             strleaf(ORCGPU_PRED_IN, "i64", nullptr, 2), intlit(1), intlit(2),
                                             cmp_node(ORCGPU_PRED_GE), T("i:5"), T("c:i32"),
                                             cmp_node(ORCGPU_PRED_EQ), T("+"), T("c:p"), T("c:q"), T("c:w")};
  five[5].value_type = 0;
  {
    FilterPlan plan;
    const int rc = compile(five, kFlat, plan);
    printf("five %d\n", rc);
    dump("planes", plan);
    // every expression leaf's blob parses, and names planes inside the plan's
    for (uint32_t k : plan.expr_leaves) {
      FilterExprBlob e;
      const FilterInsn& in = plan.prog[k];
      printf("blob %u %d %d\n", k, (int)filter_expr_blob(plan.lits.data() + in.lit_off, in.lit_len, &e), (int)((size_t)in.i + 1 < plan.n_planes()));
    }
    // ---- filter_plan_append: a condition with an expression leaf (and a LIKE) behind a row filter that has both as well ----
    FilterPlan cond;
    std::vector<orcgpu_predicate_node> c = {enode(ORCGPU_PRED_AND, 2), cmp_node(ORCGPU_PRED_NE), T("*"), T("c:f64"), T("c:g64"), T("f:3ff0000000000000"),
                                            strleaf(ORCGPU_PRED_LIKE, "vc", "%x")};
    printf("cond %d\n", compile(c, kFlat, cond));
    dump("cond_planes", cond);
    plan.lits.push_back(0);  // (the pool need not end on a boundary: the append pads)
    const uint32_t first = filter_plan_append(plan, cond);
    printf("merged_first %u\n", first);
    dump("merged", plan);
    std::vector<FilterExprRead> reads;
    for (uint32_t k : plan.expr_leaves) {
      FilterExprBlob e;
      const FilterInsn& in = plan.prog[k];
      printf("blob %u %d %d\n", k, (int)filter_expr_blob(plan.lits.data() + in.lit_off, in.lit_len, &e), (int)((size_t)in.i + 1 < plan.n_planes()));
      filter_expr_reads(plan, in, reads);
    }
    printf("reads");
    for (const FilterExprRead& r : reads) printf(" %s:%u", kColumns[r.col].name, r.kind);
    printf("\n");
  }
  return 0;
}
