// computed_check.cpp -- the computed columns' plan (orc_rust_amd/csrc/orcgpu_computed_plan.inc) and the interpreter the kernel runs
// (orc_rust_amd/csrc/device/agg_expr_eval.h), the very text liborcgpu.so is built from, under AddressSanitizer + UBSan on the CPU
// (TEST INFRASTRUCTURE).  Builds its own cases and prints one line per fact; tests/test_computed_host_sanitized.py holds the lines
// to include/orcgpu.h and to tests/computed_model.py.
//   plan <name> <status> <n columns> <n ops> then per column <cls>:<scale>:<first op>:<n ops>:<reads>\t<message>
//   eval <name> <state: 0 null, 1 value, 2 overflow> <value: int, or the double's bits in hex>
// The columns of every case: a, b Long; d Date; p Decimal(.., 2); q Decimal(.., 10); w Decimal(.., 0); x, y Double; s String;
// t Boolean; ts Timestamp; st a Struct (nested).  `eval` lines take the operands' values from the command line: name=value ...
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/orcgpu.h"
#include "../../orc_rust_amd/csrc/orcgpu_computed_plan.inc"

using namespace orcgpu_host;

static const char* kNames[] = {"a", "b", "d", "p", "q", "w", "x", "y", "s", "t", "ts", "st"};
static const int32_t kTypes[] = {ORCGPU_T_LONG, ORCGPU_T_LONG, ORCGPU_T_DATE, ORCGPU_T_DECIMAL, ORCGPU_T_DECIMAL, ORCGPU_T_DECIMAL, ORCGPU_T_DOUBLE, ORCGPU_T_DOUBLE,
                                 ORCGPU_T_STRING, ORCGPU_T_BOOLEAN, ORCGPU_T_TIMESTAMP, ORCGPU_T_STRUCT};
static const uint32_t kScales[] = {0, 0, 0, 2, 10, 0, 0, 0, 0, 0, 0, 0};
constexpr uint32_t kN = 12;

static std::vector<AggExprCol> columns(bool dict_s = false) {
  std::vector<AggExprCol> c(kN);
  for (uint32_t k = 0; k < kN; k++) {
    c[k].orc_type = kTypes[k];
    c[k].scale = kScales[k];
    const int cls = agg_class(kTypes[k]);
    c[k].fkind = cls == ACLASS_FLOAT ? FKIND_FLOAT : cls == ACLASS_DEC ? FKIND_DEC128 : (cls == ACLASS_INT || cls == ACLASS_DATE) ? FKIND_INT : FKIND_OTHER;
    c[k].dict_out = dict_s && kTypes[k] == ORCGPU_T_STRING;
  }
  return c;
}

// An expression in pre-order, one token a node: c:<column>  i:<int64>  f:<double>  + - * neg
struct Expr {
  std::vector<orcgpu_agg_expr_node> nodes;
  std::vector<std::string> keep;
  orcgpu_agg_expr view() const { return {nodes.data(), (uint32_t)nodes.size()}; }
};
static Expr parse(const char* text) {
  Expr e;
  std::vector<std::string> toks;
  std::string cur;
  for (const char* p = text;; p++) {
    if (*p == ' ' || !*p) {
      if (!cur.empty()) toks.push_back(cur);
      cur.clear();
      if (!*p) break;
    } else cur += *p;
  }
  e.keep.reserve(toks.size());
  for (const std::string& t : toks) {
    orcgpu_agg_expr_node n;
    memset(&n, 0, sizeof(n));
    if (t.rfind("c:", 0) == 0) {
      e.keep.push_back(t.substr(2));
      n.op = ORCGPU_AGG_EXPR_COLUMN;
      n.column = e.keep.back().c_str();
    } else if (t.rfind("i:", 0) == 0) {
      n.op = ORCGPU_AGG_EXPR_LITERAL;
      n.value_type = ORCGPU_PV_INT64;
      n.i = strtoll(t.c_str() + 2, nullptr, 10);
    } else if (t.rfind("f:", 0) == 0) {
      n.op = ORCGPU_AGG_EXPR_LITERAL;
      n.value_type = ORCGPU_PV_FLOAT64;
      n.f = strtod(t.c_str() + 2, nullptr);
    } else n.op = t == "+" ? ORCGPU_AGG_EXPR_ADD : t == "-" ? ORCGPU_AGG_EXPR_SUB : t == "*" ? ORCGPU_AGG_EXPR_MUL : ORCGPU_AGG_EXPR_NEG;
    e.nodes.push_back(n);
  }
  return e;
}

static int compile(const std::vector<std::pair<std::string, std::string>>& cols, ComputedPlan& plan, bool dict_s = false, uint32_t n_proj = kN - 1) {
  std::vector<Expr> es;
  std::vector<const char*> names;
  std::vector<orcgpu_agg_expr> views;
  for (auto& c : cols) es.push_back(parse(c.second.c_str()));
  for (size_t k = 0; k < cols.size(); k++) {
    names.push_back(cols[k].first.c_str());
    views.push_back(es[k].view());
  }
  const std::vector<AggExprCol> xc = columns(dict_s);
  std::vector<uint8_t> nested(kN, 0);
  nested[kN - 1] = 1;  // st
  return computed_compile(names.data(), views.data(), (uint32_t)names.size(), kNames, kN, kNames, xc.data(), nested.data(), n_proj, plan);  // (n_proj = kN: with the Struct)
}

static void plan_line(const char* name, const std::vector<std::pair<std::string, std::string>>& cols, bool dict_s = false, uint32_t n_proj = kN - 1) {
  ComputedPlan plan;
  const int rc = compile(cols, plan, dict_s, n_proj);
  printf("plan %s %d %zu %zu", name, rc, plan.cols.size(), plan.ops.size());
  for (const ComputedColumn& c : plan.cols) printf(" %u:%d:%u:%u:%zu", c.cls, c.scale, c.first_op, c.n_ops, c.reads.size());
  printf("\t%s\n", plan.err);
}

static void print_i128(agg_i128 v) {
  if (v == 0) {
    printf("0");
    return;
  }
  const bool neg = v < 0;
  agg_u128 m = neg ? (agg_u128)0 - (agg_u128)v : (agg_u128)v;
  char buf[48];
  int n = 0;
  while (m) {
    buf[n++] = (char)('0' + (int)(m % 10));
    m /= 10;
  }
  if (neg) putchar('-');
  while (n) putchar(buf[--n]);
}
static agg_i128 parse_i128(const char* s) {
  const bool neg = *s == '-';
  if (neg) s++;
  agg_u128 m = 0;
  for (; *s; s++) m = m * 10 + (agg_u128)(*s - '0');
  return (agg_i128)(neg ? (agg_u128)0 - m : m);
}

// the operands of one row, by name; absent: NULL
struct Row {
  std::map<std::string, std::string> v;
  bool valid(uint32_t col) const { return v.count(kNames[col]) != 0; }
  agg_i128 load_int(uint32_t col) const { return parse_i128(v.at(kNames[col]).c_str()); }
  agg_i128 load_dec(uint32_t col) const { return load_int(col); }
  double load_f64(uint32_t col) const { return agg_f64_of_bits(strtoull(v.at(kNames[col]).c_str(), nullptr, 16)); }
};

// eval <name> "<expression>" name=value ...: the kernel's own steps -- the interpreter, then the range of the output type
static void eval_line(const char* name, const char* text, int argc, char** argv, int first) {
  ComputedPlan plan;
  const int rc = compile({{"r", text}}, plan);
  if (rc) {
    printf("eval %s refused %d\t%s\n", name, rc, plan.err);
    return;
  }
  Row row;
  for (int k = first; k < argc && strchr(argv[k], '='); k++) {
    const std::string kv = argv[k];
    row.v[kv.substr(0, kv.find('='))] = kv.substr(kv.find('=') + 1);
  }
  const ComputedColumn& c = plan.cols[0];
  const AggExprOp* prog = plan.ops.data() + c.first_op;
  if (c.cls == XCLASS_FLOAT) {
    double f = 0.0;
    const int st = agg_expr_eval_f64(prog, c.n_ops, row, &f);
    printf("eval %s %d %llx\n", name, st, st == AGG_ROW_VALUE ? agg_bits_of_f64(f) : 0ull);
    return;
  }
  agg_i128 v = 0;
  int st = agg_expr_eval_i128(prog, c.n_ops, row, &v);
  if (st == AGG_ROW_VALUE && c.cls == XCLASS_INT && v != (agg_i128)(long long)v) st = AGG_ROW_OVERFLOW;
  if (st == AGG_ROW_VALUE && c.cls == XCLASS_DEC && (v >= agg_pow10(38) || v <= -agg_pow10(38))) st = AGG_ROW_OVERFLOW;
  printf("eval %s %d ", name, st);
  print_i128(st == AGG_ROW_VALUE ? v : 0);
  printf("\n");
}

int main(int argc, char** argv) {
  // eval cases from the command line: eval <name> <expression> name=value ...
  for (int k = 1; k < argc; k++)
    if (strcmp(argv[k], "eval") == 0 && k + 2 < argc) eval_line(argv[k + 1], argv[k + 2], argc, argv, k + 3);
  // the plan for each class, and the program table's layout
  plan_line("int", {{"r", "+ c:a c:b"}});
  plan_line("date", {{"r", "- c:d c:a"}});
  plan_line("dec_2x2", {{"r", "* c:p c:p"}});
  plan_line("dec_rev", {{"r", "* c:p - i:1 c:q"}});
  plan_line("float", {{"r", "+ * c:x c:y f:0.5"}});
  plan_line("three", {{"r1", "+ c:a c:b"}, {"r2", "* c:p c:q"}, {"r3", "neg c:x"}});
  plan_line("eight", {{"c0", "+ c:a i:0"}, {"c1", "+ c:a i:1"}, {"c2", "+ c:a i:2"}, {"c3", "+ c:a i:3"}, {"c4", "+ c:a i:4"}, {"c5", "+ c:a i:5"}, {"c6", "+ c:a i:6"}, {"c7", "+ c:a i:7"}});
  // names
  plan_line("nine", {{"c0", "c:a"}, {"c1", "c:a"}, {"c2", "c:a"}, {"c3", "c:a"}, {"c4", "c:a"}, {"c5", "c:a"}, {"c6", "c:a"}, {"c7", "c:a"}, {"c8", "c:a"}});
  plan_line("empty_name", {{"", "c:a"}});
  plan_line("twice", {{"r", "c:a"}, {"r", "c:b"}});
  plan_line("root_name", {{"q", "c:a"}});
  plan_line("root_name_unprojected", {{"st", "c:a"}});
  // the expressions' refusals, each naming the computed column
  plan_line("string", {{"r", "+ c:s i:1"}});
  plan_line("boolean", {{"r", "+ c:t i:1"}});
  plan_line("timestamp", {{"r", "+ c:ts i:1"}});
  plan_line("dictionary", {{"r", "+ c:s i:1"}}, true);
  plan_line("nested_projection", {{"r", "+ c:a i:1"}}, false, kN);
  plan_line("computed_operand", {{"r", "+ c:a i:1"}, {"u", "+ c:r i:1"}});
  plan_line("no_column", {{"r", "+ i:1 i:2"}});
  plan_line("unknown", {{"r", "+ c:nope i:1"}});
  plan_line("mixed", {{"r", "+ c:x c:a"}});
  plan_line("scale_40", {{"r", "* * * c:q c:q c:q c:q"}});
  plan_line("no_nodes", {{"r", ""}});
  return 0;
}
