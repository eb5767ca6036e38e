// div_check.cpp -- division in an expression (include/orcgpu.h: DIVISION): the checked divide and the interpreter (orc_rust_amd/csrc/
// device/agg_expr_eval.h) and the compiler (orc_rust_amd/csrc/orcgpu_agg_expr.inc, through the computed columns' plan, directly in
// the aggregates' mode, and as the two sides of a row filter's leaf), the very text liborcgpu.so is built from, under
// AddressSanitizer + UBSan on the CPU (TEST INFRASTRUCTURE).  Prints one line per fact; tests/test_div_host_sanitized.py holds the
// lines to tests/div_model.py.
//   div <n> <ok> <value>            for line n of the file argv[1]: "<mode 0 round, 1 floor, 2 mod> <a> <b> <k>" (round: a * 10^k / b)
//   fdiv <n> <bits>                 for line n of the file argv[2]: "<bits of a> <bits of b>", hexadecimal: the double division
//   plan <name> <status> <class> <scale> <n ops> <op>:<col>:<lo> ...\t<message>   (computed-column mode: a Date is days everywhere)
//   agg <name> <status> <kind> <scale> <n ops>\t<message>                        (aggregate mode)
//   pair <name> <status> <class> <left scale> <right scale> <n left ops> <n right ops>\t<message>   (a filter leaf's two sides)
//   eval <name> <state: 0 null, 1 value, 2 overflow> <value>          for every `eval <name> <expression> <column>=<value> ...` of argv
// (a `plan <name> <expression>` of argv is printed like the plans listed in main)
// The columns: a, b Long; i Int; d Date; p Decimal(.., 2); q Decimal(.., 4); x, y Double; s String.
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

static const char* kNames[] = {"a", "b", "i", "d", "p", "q", "x", "y", "s"};
static const int32_t kTypes[] = {ORCGPU_T_LONG, ORCGPU_T_LONG, ORCGPU_T_INT, ORCGPU_T_DATE, ORCGPU_T_DECIMAL, ORCGPU_T_DECIMAL, ORCGPU_T_DOUBLE, ORCGPU_T_DOUBLE, ORCGPU_T_STRING};
static const uint32_t kScales[] = {0, 0, 0, 0, 2, 4, 0, 0, 0};
constexpr uint32_t kN = 9;

static std::vector<AggExprCol> columns() {
  std::vector<AggExprCol> c(kN);
  for (uint32_t k = 0; k < kN; k++) {
    c[k].orc_type = kTypes[k];
    c[k].scale = kScales[k];
    const int cls = agg_class(kTypes[k]);
    c[k].fkind = cls == ACLASS_FLOAT ? FKIND_FLOAT : cls == ACLASS_DEC ? FKIND_DEC128 : (cls == ACLASS_INT || cls == ACLASS_DATE) ? FKIND_INT : FKIND_OTHER;
  }
  return c;
}

static agg_i128 parse_i128(const char* s) {
  const bool neg = *s == '-';
  if (neg) s++;
  agg_u128 m = 0;
  for (; *s >= '0' && *s <= '9'; s++) m = m * 10 + (agg_u128)(*s - '0');
  return (agg_i128)(neg ? (agg_u128)0 - m : m);
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

// An expression in pre-order, one token a node: c:<column>  i:<int64>  f:<double>  dec:<unscaled>:<scale>  + - * neg  / // %
// /:<i> (a division with the node's i)  year (a date part)  op:<n> (a node of op n)
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
    } else if (t.rfind("dec:", 0) == 0) {
      const agg_i128 v = parse_i128(t.c_str() + 4);
      e.keep.push_back(std::string((const char*)&v, 16));
      n.op = ORCGPU_AGG_EXPR_LITERAL;
      n.value_type = ORCGPU_PV_DECIMAL128;
      n.s = e.keep.back().data();
      n.s_len = 16;
      n.i = strtoll(strchr(t.c_str() + 4, ':') + 1, nullptr, 10);
    } else if (t.rfind("/:", 0) == 0) {
      n.op = ORCGPU_AGG_EXPR_DIV;
      n.i = strtoll(t.c_str() + 2, nullptr, 10);
    } else if (t.rfind("op:", 0) == 0) {
      n.op = (uint32_t)strtoul(t.c_str() + 3, nullptr, 10);
    } else if (t == "/") {
      n.op = ORCGPU_AGG_EXPR_DIV;
      n.i = -1;
    } else if (t == "year") {
      n.op = ORCGPU_AGG_EXPR_DATE_PART;
      n.i = ORCGPU_DATE_PART_YEAR;
    } else {
      n.op = t == "+" ? ORCGPU_AGG_EXPR_ADD : t == "-" ? ORCGPU_AGG_EXPR_SUB : t == "*" ? ORCGPU_AGG_EXPR_MUL : t == "//" ? ORCGPU_AGG_EXPR_FLOOR_DIV
           : t == "%" ? ORCGPU_AGG_EXPR_MOD : ORCGPU_AGG_EXPR_NEG;
    }
    e.nodes.push_back(n);
  }
  return e;
}

static int compile(const char* text, ComputedPlan& plan) {
  const Expr e = parse(text);
  const char* name = "r";
  const orcgpu_agg_expr view = e.view();
  const std::vector<AggExprCol> xc = columns();
  std::vector<uint8_t> nested(kN, 0);
  return computed_compile(&name, &view, 1, kNames, kN, kNames, xc.data(), nested.data(), kN, plan);
}

static void plan_line(const char* name, const char* text) {
  ComputedPlan plan;
  const int rc = compile(text, plan);
  printf("plan %s %d", name, rc);
  if (!rc) {
    const ComputedColumn& c = plan.cols[0];
    printf(" %u %d %u", c.cls, c.scale, c.n_ops);
    for (uint32_t k = 0; k < c.n_ops; k++) {
      const AggExprOp& o = plan.ops[c.first_op + k];
      // (an AX_DIV's 10^k in full; everything else by its low word, signed)
      if (o.op == AX_DIV) {
        printf(" %u:%u:", o.op, o.col);
        print_i128(agg_i128_of(o.lo, o.hi));
      } else printf(" %u:%u:%lld", o.op, o.col, (long long)o.lo);
    }
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

// the two sides of a row filter's leaf, typed together
static void pair_line(const char* name, const char* lhs, const char* rhs) {
  const Expr l = parse(lhs), r = parse(rhs);
  const orcgpu_agg_expr lv = l.view(), rv = r.view();
  const std::vector<AggExprCol> xc = columns();
  char err[384] = "";
  AggExprCompiler x{kNames, xc.data(), kN, "a comparison", err, sizeof(err)};
  x.predicate = true;
  AggExprCompiler::Side ls, rs;
  const int rc = x.compile_pair(&lv, &rv, ls, rs);
  printf("pair %s %d %d %d %d %zu %zu\t%s\n", name, rc, x.cls, ls.scale, rs.scale, ls.ops.size(), rs.ops.size(), err);
}

// the operands of one row, by name; absent: NULL
struct Row {
  std::map<std::string, agg_i128> v;
  bool valid(uint32_t col) const { return v.count(kNames[col]) != 0; }
  agg_i128 load_int(uint32_t col) const { return v.at(kNames[col]); }
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
    row.v[kv.substr(0, kv.find('='))] = parse_i128(kv.c_str() + kv.find('=') + 1);
  }
  const ComputedColumn& c = plan.cols[0];
  agg_i128 v = 0;
  int st = agg_expr_eval_i128(plan.ops.data() + c.first_op, c.n_ops, row, &v);
  // the instantiation without the divide never hands out a value for a program that holds a division
  agg_i128 w = 0;
  const int st0 = agg_expr_eval_i128_as<false>(plan.ops.data() + c.first_op, c.n_ops, row, &w);
  if (agg_ops_hold_division(plan.ops.data() + c.first_op, c.n_ops) ? st0 == AGG_ROW_VALUE : (st0 != st || (st == AGG_ROW_VALUE && v != w))) {
    printf("eval %s broken-without-divide %d\n", name, st0);
    return;
  }
  if (st == AGG_ROW_VALUE && c.cls == XCLASS_INT && v != (agg_i128)(long long)v) st = AGG_ROW_OVERFLOW;
  if (st == AGG_ROW_VALUE && c.cls == XCLASS_DEC && (v >= agg_pow10(38) || v <= -agg_pow10(38))) st = AGG_ROW_OVERFLOW;
  printf("eval %s %d ", name, st);
  print_i128(st == AGG_ROW_VALUE ? v : 0);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  {
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    char a[64], b[64];
    unsigned mode, k, n = 0;
    while (fscanf(f, "%u %63s %63s %u", &mode, a, b, &k) == 4) {
      agg_i128 r = 0;
      const bool ok = mode == AGG_DIV_ROUND ? agg_div_scaled_checked(parse_i128(a), agg_pow10(k), parse_i128(b), &r) : agg_div_checked(parse_i128(a), parse_i128(b), mode, &r);
      printf("div %u %d ", n++, ok ? 1 : 0);
      print_i128(r);
      printf("\n");
    }
    fclose(f);
  }
  {
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    unsigned long long a, b;
    unsigned n = 0;
    while (fscanf(f, "%llx %llx", &a, &b) == 2) printf("fdiv %u %llx\n", n++, agg_bits_of_f64(agg_f64_div(agg_f64_of_bits(a), agg_f64_of_bits(b))));
    fclose(f);
  }
  for (int k = 3; k < argc; k++)
    if (strcmp(argv[k], "eval") == 0 && k + 2 < argc) eval_line(argv[k + 1], argv[k + 2], argc, argv, k + 3);
    else if (strcmp(argv[k], "plan") == 0 && k + 2 < argc) plan_line(argv[k + 1], argv[k + 2]);
  // the plans: the ops, the class change, the scale rule
  plan_line("int_by_int", "/ c:a c:b");
  plan_line("dec_by_int", "/ c:p c:a");
  plan_line("dec_by_dec", "/ c:p c:q");
  plan_line("scale_0", "/:0 c:q c:q");
  plan_line("scale_38", "/:38 c:a c:b");
  plan_line("high_scale_default", "/ * * * * * * * * c:q c:q c:q c:q c:q c:q c:q c:q c:q c:a");
  plan_line("floor", "// c:a c:i");
  plan_line("mod", "% c:d i:7");
  plan_line("int_stays_int", "+ // c:a i:16 % c:a i:16");
  plan_line("mod_in_dec", "* % year c:d i:100 c:p");
  plan_line("sum_of_quotients", "+ / c:p c:a c:q");
  plan_line("float", "/ c:x c:y");
  plan_line("float_scale_unread", "/:3 c:x + c:y f:1");
  // the reversed order: the right child needs more slots and goes first, ONE swap in front of the op
  plan_line("reversed_div", "/ c:a + c:b c:i");
  plan_line("reversed_floor", "// c:a + c:b c:i");
  plan_line("reversed_mod", "% c:a + c:b c:i");
  plan_line("reversed_float", "/ c:x * c:y c:y");
  plan_line("not_reversed", "/ + c:b c:i c:a");
  // the slots and the depth count: a division is binary
  plan_line("deep_4", "/ + / c:a c:b / c:a c:b + / c:a c:b / c:a c:b");
  plan_line("deep_5", "/ / / / c:a c:b / c:a c:b / / c:a c:b / c:a c:b / / / c:a c:b / c:a c:b / / c:a c:b / c:a c:b");
  // the folding, with the evaluator's own functions; one that overflows is left to the rows
  plan_line("folded_div", "+ c:p / i:1 i:3");
  plan_line("folded_half", "+ c:a /:0 i:-5 i:2");
  plan_line("folded_floor_mod", "+ c:a + // i:-7 i:2 % i:-7 i:2");
  plan_line("folded_float", "+ c:x / f:1 f:3");
  plan_line("folded_float_zero", "+ c:x / f:1 f:0");
  plan_line("not_folded_zero", "+ c:a // i:1 i:0");
  plan_line("not_folded_mod_zero", "+ c:a % i:1 i:0");
  plan_line("not_folded_div_zero", "+ c:p / dec:150:2 i:0");
  plan_line("not_folded_product", "+ c:p /:38 i:9223372036854775807 i:3");
  // the refusals
  plan_line("bad_scale_39", "/:39 c:a c:b");
  plan_line("bad_scale_minus_2", "/:-2 c:a c:b");
  plan_line("k_negative", "/:1 c:q c:a");
  plan_line("k_past_38", "/ c:p /:38 c:a c:b");
  plan_line("floor_of_decimal", "// c:p i:2");
  plan_line("mod_by_decimal", "% c:a c:q");
  plan_line("mod_of_quotient", "% / c:a c:b i:2");
  plan_line("floor_in_float", "// c:x f:2");
  plan_line("mod_in_float", "% c:x c:y");
  plan_line("float_beside_exact", "/ c:x c:a");
  plan_line("string_operand", "/ c:s i:2");
  plan_line("year_of_quotient", "year / c:d i:7");
  plan_line("year_of_integer_quotient", "year /:0 c:d i:7");
  plan_line("no_operand", "/ c:a");
  plan_line("unknown_20", "op:20 c:a c:b");
  // the aggregates' mode
  agg_line("sum_unit_price", "/ c:p c:a");
  agg_line("sum_int_quotient", "/ c:a c:b");
  agg_line("sum_mod", "% c:a i:16");
  agg_line("sum_float", "/ c:x c:y");
  agg_line("date_outside", "// c:d i:7");
  agg_line("literals_alone", "/ i:1 i:2");
  // a filter leaf: the class is decided over both sides together
  pair_line("quotient_against_int", "/ c:a c:b", "i:2");
  pair_line("int_against_quotient", "c:a", "/ c:p i:3");
  pair_line("mod_against_int", "% c:a i:16", "i:3");
  pair_line("float_pair", "/ c:x c:y", "f:0.5");
  pair_line("floor_beside_float", "// c:a i:2", "c:x");
  return 0;
}
