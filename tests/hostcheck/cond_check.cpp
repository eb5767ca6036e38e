// cond_check.cpp -- the conditionals of an expression (include/orcgpu.h: CONDITIONALS): the compiler (orc_rust_amd/csrc/
// orcgpu_agg_expr.inc, through the computed columns' plan, in the aggregates' mode, and as the two sides of a row filter's leaf) and the
// interpreter with the conditionals (orc_rust_amd/csrc/device/agg_expr_eval.h), the very text liborcgpu.so is built from, under
// AddressSanitizer + UBSan on the CPU (TEST INFRASTRUCTURE).  Prints one line per fact; tests/test_cond_host_sanitized.py holds the
// lines to tests/cond_model.py.
//   plan <name> <status> <class> <scale> <n ops> <op>:<col>:<lo> ...\t<message>   (computed-column mode: a Date is days everywhere)
//   agg <name> <status> <kind> <scale> <n ops>\t<message>                        (aggregate mode)
//   pair <name> <status> <class> <left scale> <right scale> <n left ops> <n right ops> <left holds a conditional> <right ...>\t<message>
//   eval <name> <state: 0 null, 1 value, 2 overflow> <value, a double as its bits in hexadecimal>
//        for every `eval <name> <expression> <column>=<value> ...` of argv (a double column: its bits, hexadecimal; absent: NULL);
//        `eval <name> old-interpreter-gave-a-value ..` instead where an instantiation WITHOUT the conditionals, handed a program that
//        holds one, did not overflow the row (INT / DEC) or give NaN (FLOAT)
//   bits <name> <nul> <ovf>       the two masks after a fixed sequence of push / merge / merge3 / swap with four slots in use
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

// An expression in pre-order, one token a node: c:<column>  i:<int64>  f:<bits of a double, hexadecimal>  dec:<unscaled>:<scale>
// + - * neg / // % year   if coalesce abs null cmp:<0 .. 5> isnull and or not   op:<n> (a node of op n)
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
  static const std::map<std::string, uint32_t> plain = {
      {"+", ORCGPU_AGG_EXPR_ADD}, {"-", ORCGPU_AGG_EXPR_SUB}, {"*", ORCGPU_AGG_EXPR_MUL}, {"neg", ORCGPU_AGG_EXPR_NEG}, {"//", ORCGPU_AGG_EXPR_FLOOR_DIV},
      {"%", ORCGPU_AGG_EXPR_MOD}, {"if", ORCGPU_AGG_EXPR_IF}, {"coalesce", ORCGPU_AGG_EXPR_COALESCE}, {"abs", ORCGPU_AGG_EXPR_ABS}, {"null", ORCGPU_AGG_EXPR_NULL},
      {"isnull", ORCGPU_AGG_EXPR_IS_NULL}, {"and", ORCGPU_AGG_EXPR_AND}, {"or", ORCGPU_AGG_EXPR_OR}, {"not", ORCGPU_AGG_EXPR_NOT}};
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
      n.f = agg_f64_of_bits(strtoull(t.c_str() + 2, nullptr, 16));
    } else if (t.rfind("dec:", 0) == 0) {
      const agg_i128 v = parse_i128(t.c_str() + 4);
      e.keep.push_back(std::string((const char*)&v, 16));
      n.op = ORCGPU_AGG_EXPR_LITERAL;
      n.value_type = ORCGPU_PV_DECIMAL128;
      n.s = e.keep.back().data();
      n.s_len = 16;
      n.i = strtoll(strchr(t.c_str() + 4, ':') + 1, nullptr, 10);
    } else if (t.rfind("cmp:", 0) == 0) {
      n.op = ORCGPU_AGG_EXPR_CMP;
      n.i = strtoll(t.c_str() + 4, nullptr, 10);
    } else if (t.rfind("op:", 0) == 0) {
      n.op = (uint32_t)strtoul(t.c_str() + 3, nullptr, 10);
    } else if (t == "/") {
      n.op = ORCGPU_AGG_EXPR_DIV;
      n.i = -1;
    } else if (t == "year") {
      n.op = ORCGPU_AGG_EXPR_DATE_PART;
      n.i = ORCGPU_DATE_PART_YEAR;
    } else if (plain.count(t)) {
      n.op = plain.at(t);
    } else {
      fprintf(stderr, "cond_check: the token '%s'\n", t.c_str());
      exit(2);
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
      printf(" %u:%u:%lld", o.op, o.col, (long long)o.lo);
    }
  }
  printf("\t%s\n", plan.err);
}

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

static void pair_line(const char* name, const char* lhs, const char* rhs) {
  const Expr l = parse(lhs), r = parse(rhs);
  const orcgpu_agg_expr lv = l.view(), rv = r.view();
  const std::vector<AggExprCol> xc = columns();
  char err[384] = "";
  AggExprCompiler x{kNames, xc.data(), kN, "a comparison", err, sizeof(err)};
  x.predicate = true;
  AggExprCompiler::Side ls, rs;
  const int rc = x.compile_pair(&lv, &rv, ls, rs);
  printf("pair %s %d %d %d %d %zu %zu %d %d\t%s\n", name, rc, x.cls, ls.scale, rs.scale, ls.ops.size(), rs.ops.size(),
         (int)agg_ops_hold_conditional(ls.ops.data(), ls.ops.size()), (int)agg_ops_hold_conditional(rs.ops.data(), rs.ops.size()), err);
}

// the operands of one row, by name; absent: NULL.  A NULL's value is poison: the interpreter must not let it show.
struct Row {
  std::map<std::string, agg_i128> v;
  std::map<std::string, double> f;
  bool valid(uint32_t col) const { return v.count(kNames[col]) != 0 || f.count(kNames[col]) != 0; }
  agg_i128 load_int(uint32_t col) const { return v.count(kNames[col]) ? v.at(kNames[col]) : agg_i128_of(0xdeadbeefdeadbeefull, 0x7badbeefdeadbeefull); }
  agg_i128 load_dec(uint32_t col) const { return load_int(col); }
  double load_f64(uint32_t col) const { return f.count(kNames[col]) ? f.at(kNames[col]) : agg_f64_of_bits(0x7ff8dead00000000ull); }
};

static void eval_line(const char* name, const char* text, int argc, char** argv, int first) {
  ComputedPlan plan;
  const int rc = compile(text, plan);
  if (rc) {
    printf("eval %s refused %d\t%s\n", name, rc, plan.err);
    return;
  }
  Row row;
  for (int k = first; k < argc && strchr(argv[k], '='); k++) {
    const std::string kv = argv[k], key = kv.substr(0, kv.find('='));
    if (key == "x" || key == "y") row.f[key] = agg_f64_of_bits(strtoull(kv.c_str() + kv.find('=') + 1, nullptr, 16));
    else row.v[key] = parse_i128(kv.c_str() + kv.find('=') + 1);
  }
  const ComputedColumn& c = plan.cols[0];
  const AggExprOp* prog = plan.ops.data() + c.first_op;
  const bool cond = agg_ops_hold_conditional(prog, c.n_ops);
  if (c.cls == XCLASS_FLOAT) {
    double v = 0.0;
    const int st = cond ? agg_expr_eval_f64_as<true, true>(prog, c.n_ops, row, &v) : agg_expr_eval_f64_as<true>(prog, c.n_ops, row, &v);
    if (cond) {  // the instantiations without the conditionals: NaN, as a division's result is without the divide -- or the row is NULL
      double w0 = 0.0, w1 = 0.0;
      const int s0 = agg_expr_eval_f64_as<false>(prog, c.n_ops, row, &w0), s1 = agg_expr_eval_f64_as<true>(prog, c.n_ops, row, &w1);
      if ((s0 != AGG_ROW_NULL && w0 == w0) || (s1 != AGG_ROW_NULL && w1 == w1)) {
        printf("eval %s old-interpreter-gave-a-value %d %d\n", name, s0, s1);
        return;
      }
    }
    printf("eval %s %d %llx\n", name, st, st == AGG_ROW_VALUE ? agg_bits_of_f64(v) : 0ull);
    return;
  }
  agg_i128 v = 0;
  int st = cond ? agg_expr_eval_i128_as<true, true>(prog, c.n_ops, row, &v) : agg_expr_eval_i128_as<true>(prog, c.n_ops, row, &v);
  if (cond) {  // the instantiations without the conditionals never hand out a value for it: the mark overflows the row
    agg_i128 w = 0;
    const int s0 = agg_expr_eval_i128_as<false>(prog, c.n_ops, row, &w), s1 = agg_expr_eval_i128_as<true>(prog, c.n_ops, row, &w);
    if (s0 != AGG_ROW_OVERFLOW || s1 != AGG_ROW_OVERFLOW) {
      printf("eval %s old-interpreter-gave-a-value %d %d\n", name, s0, s1);
      return;
    }
  }
  if (st == AGG_ROW_VALUE && c.cls == XCLASS_INT && v != (agg_i128)(long long)v) st = AGG_ROW_OVERFLOW;
  if (st == AGG_ROW_VALUE && c.cls == XCLASS_DEC && (v >= agg_pow10(38) || v <= -agg_pow10(38))) st = AGG_ROW_OVERFLOW;
  printf("eval %s %d ", name, st);
  print_i128(st == AGG_ROW_VALUE ? v : 0);
  printf("\n");
}

int main(int argc, char** argv) {
  for (int k = 1; k < argc; k++)
    if (strcmp(argv[k], "eval") == 0 && k + 2 < argc) eval_line(argv[k + 1], argv[k + 2], argc, argv, k + 3);
    else if (strcmp(argv[k], "plan") == 0 && k + 2 < argc) plan_line(argv[k + 1], argv[k + 2]);
    else if (strcmp(argv[k], "agg") == 0 && k + 2 < argc) agg_line(argv[k + 1], argv[k + 2]);
    else if (strcmp(argv[k], "pair") == 0 && k + 3 < argc) pair_line(argv[k + 1], argv[k + 2], argv[k + 3]);
  // the bit masks with all four slots in use: push N, push -, push O, push N -> merge(-, O) -> swap -> push(N) -> merge3(O) -> swap
  {
    AggSlotBits m = {0, 0};
    m.push(true, false);
    m.push(false, false);
    m.push(false, true);
    m.push(true, false);
    printf("bits four %u %u\n", m.nul, m.ovf);  // top first: N O - N
    m.merge(false, true);                       // O - N
    printf("bits merged %u %u\n", m.nul, m.ovf);
    m.swap();                                   // - O N
    printf("bits swapped %u %u\n", m.nul, m.ovf);
    m.push(true, false);                        // N - O N
    printf("bits pushed %u %u\n", m.nul, m.ovf);
    m.merge3(false, true);                      // O N
    printf("bits merged3 %u %u\n", m.nul, m.ovf);
    m.swap();                                   // N O
    m.set(false, false);                        // - O
    printf("bits set %u %u\n", m.nul, m.ovf);
  }
  return 0;
}
