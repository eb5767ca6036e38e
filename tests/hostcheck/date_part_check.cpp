// date_part_check.cpp -- the date part of an expression (include/orcgpu.h: DATE PARTS): the compiler (orc_rust_amd/csrc/
// orcgpu_agg_expr.inc, through the computed columns' plan and directly in the aggregates' mode) and the interpreter with its
// calendar function (orc_rust_amd/csrc/device/agg_expr_eval.h), the very text liborcgpu.so is built from, under AddressSanitizer +
// UBSan on the CPU (TEST INFRASTRUCTURE).  Prints one line per fact; tests/test_date_part_host_sanitized.py holds the lines to
// tests/date_part_model.py.
//   part <days> <year> <quarter> <month> <day> <day of week> <day of year>      for every `days` read from the file argv[1]
//   plan <name> <status> <class> <scale> <n ops> <op>:<col>:<lo> ...\t<message>   (computed-column mode: a Date is days everywhere)
//   agg <name> <status> <kind> <scale> <n ops>\t<message>                        (aggregate mode: a Date is days below a date part only)
//   eval <name> <state: 0 null, 1 value, 2 overflow> <value>
// The columns: a, b Long; i Int; d Date; p Decimal(.., 2); x Double; s String; t Boolean; ts Timestamp.
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

static const char* kNames[] = {"a", "b", "i", "d", "p", "x", "s", "t", "ts"};
static const int32_t kTypes[] = {ORCGPU_T_LONG, ORCGPU_T_LONG, ORCGPU_T_INT, ORCGPU_T_DATE, ORCGPU_T_DECIMAL, ORCGPU_T_DOUBLE, ORCGPU_T_STRING, ORCGPU_T_BOOLEAN, ORCGPU_T_TIMESTAMP};
static const uint32_t kScales[] = {0, 0, 0, 0, 2, 0, 0, 0, 0};
constexpr uint32_t kN = 9;

static std::vector<AggExprCol> columns(bool dict_s = false) {
  std::vector<AggExprCol> c(kN);
  for (uint32_t k = 0; k < kN; k++) {
    c[k].orc_type = kTypes[k];
    c[k].scale = kScales[k];
    const int cls = agg_class(kTypes[k]);
    c[k].fkind = cls == ACLASS_FLOAT ? FKIND_FLOAT : cls == ACLASS_DEC ? FKIND_DEC128 : (cls == ACLASS_INT || cls == ACLASS_DATE || cls == ACLASS_TS) ? FKIND_INT : FKIND_OTHER;
    c[k].dict_out = dict_s && kTypes[k] == ORCGPU_T_STRING;
  }
  return c;
}

// An expression in pre-order, one token a node: c:<column>  i:<int64>  f:<double>  dec:<unscaled>:<scale>  + - * neg
// year quarter month day dow doy (a date part)  part:<n> (a date part with the part number n)  op:<n> (a node of op n)
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
  e.keep.reserve(toks.size() * 2);
  static const char* const parts[] = {"year", "quarter", "month", "day", "dow", "doy"};
  for (const std::string& t : toks) {
    orcgpu_agg_expr_node n;
    memset(&n, 0, sizeof(n));
    bool done = false;
    for (int k = 0; k < 6 && !done; k++)
      if (t == parts[k]) {
        n.op = ORCGPU_AGG_EXPR_DATE_PART;
        n.i = k;
        done = true;
      }
    if (done) {
    } else if (t.rfind("c:", 0) == 0) {
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
    } else if (t.rfind("dec:", 0) == 0) {
      const long long unscaled = strtoll(t.c_str() + 4, nullptr, 10);
      const agg_i128 v = unscaled;
      e.keep.push_back(std::string((const char*)&v, 16));
      n.op = ORCGPU_AGG_EXPR_LITERAL;
      n.value_type = ORCGPU_PV_DECIMAL128;
      n.s = e.keep.back().data();
      n.s_len = 16;
      n.i = strtoll(strchr(t.c_str() + 4, ':') + 1, nullptr, 10);
    } else if (t.rfind("part:", 0) == 0) {
      n.op = ORCGPU_AGG_EXPR_DATE_PART;
      n.i = strtoll(t.c_str() + 5, nullptr, 10);
    } else if (t.rfind("op:", 0) == 0) {
      n.op = (uint32_t)strtoul(t.c_str() + 3, nullptr, 10);
    } else n.op = t == "+" ? ORCGPU_AGG_EXPR_ADD : t == "-" ? ORCGPU_AGG_EXPR_SUB : t == "*" ? ORCGPU_AGG_EXPR_MUL : ORCGPU_AGG_EXPR_NEG;
    e.nodes.push_back(n);
  }
  return e;
}

static int compile(const char* text, ComputedPlan& plan, bool dict_s = false) {
  const Expr e = parse(text);
  const char* name = "r";
  const orcgpu_agg_expr view = e.view();
  const std::vector<AggExprCol> xc = columns(dict_s);
  std::vector<uint8_t> nested(kN, 0);
  return computed_compile(&name, &view, 1, kNames, kN, kNames, xc.data(), nested.data(), kN, plan);
}

static void plan_line(const char* name, const char* text, bool dict_s = false) {
  ComputedPlan plan;
  const int rc = compile(text, plan, dict_s);
  printf("plan %s %d", name, rc);
  if (!rc) {
    const ComputedColumn& c = plan.cols[0];
    printf(" %u %d %u", c.cls, c.scale, c.n_ops);
    for (uint32_t k = 0; k < c.n_ops; k++) printf(" %u:%u:%lld", plan.ops[c.first_op + k].op, plan.ops[c.first_op + k].col, (long long)plan.ops[c.first_op + k].lo);
  }
  printf("\t%s\n", plan.err);
}

// the aggregates' mode: predicate = false
static void agg_line(const char* name, const char* text) {
  const Expr e = parse(text);
  const orcgpu_agg_expr view = e.view();
  const std::vector<AggExprCol> xc = columns();
  char err[384] = "";
  AggExprCompiler x{kNames, xc.data(), kN, "SUM_EXPR", err, sizeof(err)};
  std::vector<AggExprOp> ops;
  uint32_t kind = 0;
  int32_t scale = 0;
  const int rc = x.compile(&view, ops, kind, scale);
  printf("agg %s %d %u %d %zu\t%s\n", name, rc, kind, scale, ops.size(), err);
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

// the operands of one row, by name; absent: NULL
struct Row {
  std::map<std::string, long long> v;
  bool valid(uint32_t col) const { return v.count(kNames[col]) != 0; }
  agg_i128 load_int(uint32_t col) const { return (agg_i128)v.at(kNames[col]); }
  agg_i128 load_dec(uint32_t col) const { return load_int(col); }
  double load_f64(uint32_t) const { return 0.0; }
};

// eval <name> "<expression>" name=value ...: the computed columns' kernel steps -- the interpreter, then the range of the output
static void eval_line(const char* name, const char* text, int argc, char** argv, int first) {
  ComputedPlan plan;
  const int rc = compile(text, plan);
  if (rc) {
    printf("eval %s refused %d\t%s\n", name, rc, plan.err);
    return;
  }
  Row row;
  for (int k = first; k < argc && strchr(argv[k], '='); k++) {
    const std::string kv = argv[k];
    row.v[kv.substr(0, kv.find('='))] = strtoll(kv.c_str() + kv.find('=') + 1, nullptr, 10);
  }
  const ComputedColumn& c = plan.cols[0];
  agg_i128 v = 0;
  int st = agg_expr_eval_i128(plan.ops.data() + c.first_op, c.n_ops, row, &v);
  if (st == AGG_ROW_VALUE && c.cls == XCLASS_INT && v != (agg_i128)(long long)v) st = AGG_ROW_OVERFLOW;
  if (st == AGG_ROW_VALUE && c.cls == XCLASS_DEC && (v >= agg_pow10(38) || v <= -agg_pow10(38))) st = AGG_ROW_OVERFLOW;
  printf("eval %s %d ", name, st);
  print_i128(st == AGG_ROW_VALUE ? v : 0);
  printf("\n");
}

int main(int argc, char** argv) {
  // every part of the days listed in the file argv[1], one number a line
  if (argc > 1) {
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    long long d;
    while (fscanf(f, "%lld", &d) == 1) {
      printf("part %lld", d);
      for (uint32_t p = 0; p < AX_PART_N; p++) printf(" %d", agg_date_part((int32_t)d, p));
      printf("\n");
    }
    fclose(f);
  }
  for (int k = 2; k < argc; k++)
    if (strcmp(argv[k], "eval") == 0 && k + 2 < argc) eval_line(argv[k + 1], argv[k + 2], argc, argv, k + 3);
  // the plans
  plan_line("year", "year c:d");
  plan_line("yyyymm", "+ * year + c:d c:a i:100 month c:d");
  plan_line("year_times_dec", "* year c:d c:p");
  plan_line("folded", "+ c:a year i:9131");            // 1995-01-01
  plan_line("folded_all_parts", "+ c:a + + + + + year i:-1 quarter i:-1 month i:-1 day i:-1 dow i:-1 doy i:-1");
  plan_line("not_folded_overflow", "+ c:a year i:2147483648");
  plan_line("nested", "year year c:d");
  plan_line("int_operand", "doy - c:i c:a");
  // the slots: a date part over an operand that needs four, and over one that needs five
  plan_line("deep_4", "year + + + c:a c:b + c:a c:b + + c:a c:b + c:a c:b");
  plan_line("deep_5", "year + + + + c:a c:b + c:a c:b + + c:a c:b + c:a c:b + + + c:a c:b + c:a c:b + + c:a c:b + c:a c:b");
  // the refusals
  plan_line("decimal_below", "year + c:d c:p");
  plan_line("float_below", "month c:x");
  plan_line("decimal_literal_below", "year + c:d dec:150:2");
  plan_line("float_literal_below", "year + c:d f:1.5");
  plan_line("float_expression", "* c:x year i:5");
  plan_line("float_column_beside", "* c:x year c:d");
  plan_line("string_below", "year c:s");
  plan_line("boolean_below", "year c:t");
  plan_line("timestamp_below", "year c:ts");
  plan_line("dictionary_below", "year c:s", true);
  plan_line("bad_part", "part:6 c:d");
  plan_line("negative_part", "part:-1 c:d");
  plan_line("no_operand", "+ c:a year");
  plan_line("unknown_9", "op:9 c:d");
  plan_line("unknown_15", "op:15 c:d");
  plan_line("nodes_32", "year + + + + + + + + + + + + + + + c:a c:a c:a c:a c:a c:a c:a c:a c:a c:a c:a c:a c:a c:a c:a c:a");
  plan_line("nodes_33", "year year + + + + + + + + + + + + + + + c:a c:a c:a c:a c:a c:a c:a c:a c:a c:a c:a c:a c:a c:a c:a c:a");
  // the aggregates' mode: a Date is days below a date part, and refused as before outside it
  agg_line("sum_year", "year c:d");
  agg_line("sum_year_plus", "+ year + c:d i:1 c:a");
  agg_line("date_plus_1", "+ c:d i:1");
  agg_line("date_beside_year", "+ c:d year c:d");
  agg_line("year_times_dec", "* year c:d c:p");
  agg_line("timestamp_below", "year c:ts");
  agg_line("string_below", "year c:s");
  agg_line("decimal_below", "year c:p");
  agg_line("literals_alone", "year i:0");
  return 0;
}
