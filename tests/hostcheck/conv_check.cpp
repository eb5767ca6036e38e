// conv_check.cpp -- the conversions of an expression (include/orcgpu.h: CONVERSIONS): the compiler (orc_rust_amd/csrc/
// orcgpu_agg_expr.inc, through the computed columns' plan and as the two sides of a row filter's leaf) and the mixed interpreter with
// its conversion functions (orc_rust_amd/csrc/device/agg_expr_eval.h), the very text liborcgpu.so is built from, under
// AddressSanitizer + UBSan on the CPU (TEST INFRASTRUCTURE).  Reads a script -- argv[1], one command a line -- and prints one line
// per fact; tests/test_conv_host_sanitized.py holds the lines to tests/conv_model.py.
//   f tof64 <unscaled> <scale>            -> f <bits of the double, hexadecimal>
//   f todec <bits> <scale>                -> f <1 ok | 0 overflow> <unscaled>
//   f toi64 <bits>                        -> f <ok> <value>
//   f rescale <unscaled> <k> <mode>       -> f <value>
//   f fround <bits> <mode>                -> f <bits>
//   plan <name> <expression>              -> plan <name> <status> <class> <scale> <n ops> <op>:<col>:<lo>:<hi> ...\t<message>
//   pair <name> <lhs> | <rhs>             -> pair <name> <status> <class> <left scale> <right scale> <left holds a conversion> <right ..>\t<message>
//   prog <name> <expression>              the program the `row` lines behind it run (refused: `prog <name> refused <status>`)
//   row <column>=<value> ...              -> row <name> <state: 0 null, 1 value, 2 overflow> <value, a double as its bits in hexadecimal>
//                                         (a double column: its bits, hexadecimal; absent: NULL); `row <name> old-interpreter-gave-a-value`
//                                         where an interpreter WITHOUT the conversions did not overflow the row or give NaN
// An expression in pre-order, one token a node: c:<column>  i:<int64>  f:<bits>  dec:<unscaled>:<scale>  + - * neg / // % year  if
// coalesce abs null cmp:<0 .. 5> isnull and or not  cast:i cast:f cast:d<scale> round:<digits> floor ceil trunc  op:<n>:<value_type>:<i>
// The columns: a, b Long; i Int; d Date; p Decimal(.., 2); q Decimal(.., 4); x, y Double; s String; w Decimal(.., 10) -- the columns
// of cond_check.cpp in its order, then w: a program without a conversion is compared op for op with what that check printed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/orcgpu.h"
#include "../../orc_rust_amd/csrc/orcgpu_computed_plan.inc"

using namespace orcgpu_host;

static const char* kNames[] = {"a", "b", "i", "d", "p", "q", "x", "y", "s", "w"};
static const int32_t kTypes[] = {ORCGPU_T_LONG, ORCGPU_T_LONG, ORCGPU_T_INT, ORCGPU_T_DATE, ORCGPU_T_DECIMAL, ORCGPU_T_DECIMAL, ORCGPU_T_DOUBLE, ORCGPU_T_DOUBLE, ORCGPU_T_STRING, ORCGPU_T_DECIMAL};
static const uint32_t kScales[] = {0, 0, 0, 0, 2, 4, 0, 0, 0, 10};
constexpr uint32_t kN = 10;

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
static std::string text_i128(agg_i128 v) {
  if (v == 0) return "0";
  const bool neg = v < 0;
  agg_u128 m = neg ? (agg_u128)0 - (agg_u128)v : (agg_u128)v;
  std::string s;
  while (m) {
    s.insert(s.begin(), (char)('0' + (int)(m % 10)));
    m /= 10;
  }
  return neg ? "-" + s : s;
}

struct Expr {
  std::vector<orcgpu_agg_expr_node> nodes;
  std::vector<std::string> keep;
  orcgpu_agg_expr view() const { return {nodes.data(), (uint32_t)nodes.size()}; }
};
static Expr parse(const std::vector<std::string>& toks) {
  Expr e;
  e.keep.reserve(toks.size() * 2);
  static const std::map<std::string, uint32_t> plain = {
      {"+", ORCGPU_AGG_EXPR_ADD}, {"-", ORCGPU_AGG_EXPR_SUB}, {"*", ORCGPU_AGG_EXPR_MUL}, {"neg", ORCGPU_AGG_EXPR_NEG}, {"//", ORCGPU_AGG_EXPR_FLOOR_DIV},
      {"%", ORCGPU_AGG_EXPR_MOD}, {"if", ORCGPU_AGG_EXPR_IF}, {"coalesce", ORCGPU_AGG_EXPR_COALESCE}, {"abs", ORCGPU_AGG_EXPR_ABS}, {"null", ORCGPU_AGG_EXPR_NULL},
      {"isnull", ORCGPU_AGG_EXPR_IS_NULL}, {"and", ORCGPU_AGG_EXPR_AND}, {"or", ORCGPU_AGG_EXPR_OR}, {"not", ORCGPU_AGG_EXPR_NOT},
      {"floor", ORCGPU_AGG_EXPR_FLOOR}, {"ceil", ORCGPU_AGG_EXPR_CEIL}, {"trunc", ORCGPU_AGG_EXPR_TRUNC}};
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
    } else if (t.rfind("cast:", 0) == 0) {
      n.op = ORCGPU_AGG_EXPR_CAST;
      n.value_type = t[5] == 'i' ? ORCGPU_PV_INT64 : t[5] == 'f' ? ORCGPU_PV_FLOAT64 : ORCGPU_PV_DECIMAL128;
      n.i = t[5] == 'd' ? strtoll(t.c_str() + 6, nullptr, 10) : 0;
    } else if (t.rfind("round:", 0) == 0) {
      n.op = ORCGPU_AGG_EXPR_ROUND;
      n.i = strtoll(t.c_str() + 6, nullptr, 10);
    } else if (t.rfind("op:", 0) == 0) {
      n.op = (uint32_t)strtoul(t.c_str() + 3, nullptr, 10);
      const char* c1 = strchr(t.c_str() + 3, ':');
      if (c1) {
        n.value_type = (int32_t)strtol(c1 + 1, nullptr, 10);
        const char* c2 = strchr(c1 + 1, ':');
        if (c2) n.i = strtoll(c2 + 1, nullptr, 10);
      }
    } else if (t == "/") {
      n.op = ORCGPU_AGG_EXPR_DIV;
      n.i = -1;
    } else if (t == "year") {
      n.op = ORCGPU_AGG_EXPR_DATE_PART;
      n.i = ORCGPU_DATE_PART_YEAR;
    } else if (plain.count(t)) {
      n.op = plain.at(t);
    } else {
      fprintf(stderr, "conv_check: the token '%s'\n", t.c_str());
      exit(2);
    }
    e.nodes.push_back(n);
  }
  return e;
}

static int compile(const std::vector<std::string>& toks, ComputedPlan& plan) {
  const Expr e = parse(toks);
  const char* name = "r";
  const orcgpu_agg_expr view = e.view();
  const std::vector<AggExprCol> xc = columns();
  std::vector<uint8_t> nested(kN, 0);
  return computed_compile(&name, &view, 1, kNames, kN, kNames, xc.data(), nested.data(), kN, plan);
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

static void run_row(const std::string& name, const ComputedPlan& plan, const std::vector<std::string>& kvs) {
  Row row;
  for (const std::string& kv : kvs) {
    const std::string key = kv.substr(0, kv.find('='));
    if (key == "x" || key == "y") row.f[key] = agg_f64_of_bits(strtoull(kv.c_str() + kv.find('=') + 1, nullptr, 16));
    else row.v[key] = parse_i128(kv.c_str() + kv.find('=') + 1);
  }
  const ComputedColumn& c = plan.cols[0];
  const AggExprOp* prog = plan.ops.data() + c.first_op;
  const bool conv = agg_ops_hold_conversion(prog, c.n_ops);
  if (c.cls == XCLASS_FLOAT) {
    double v = 0.0;
    const int st = agg_expr_eval_f64_as<true, true, true>(prog, c.n_ops, row, &v);
    if (conv) {  // the three interpreters without the conversions: NaN (the conditional one never NULL either)
      double w0 = 0.0, w1 = 0.0, w2 = 0.0;
      const int s0 = agg_expr_eval_f64_as<false>(prog, c.n_ops, row, &w0), s1 = agg_expr_eval_f64_as<true>(prog, c.n_ops, row, &w1),
                s2 = agg_expr_eval_f64_as<true, true>(prog, c.n_ops, row, &w2);
      if (s0 != AGG_ROW_VALUE || s1 != AGG_ROW_VALUE || s2 != AGG_ROW_VALUE || w0 == w0 || w1 == w1 || w2 == w2) {
        printf("row %s old-interpreter-gave-a-value %d %d %d\n", name.c_str(), s0, s1, s2);
        return;
      }
    }
    printf("row %s %d %llx\n", name.c_str(), st, st == AGG_ROW_VALUE ? agg_bits_of_f64(v) : 0ull);
    return;
  }
  agg_i128 v = 0;
  int st = agg_expr_eval_i128_as<true, true, true>(prog, c.n_ops, row, &v);
  if (conv) {  // the three interpreters without the conversions overflow the row
    agg_i128 w = 0;
    const int s0 = agg_expr_eval_i128_as<false>(prog, c.n_ops, row, &w), s1 = agg_expr_eval_i128_as<true>(prog, c.n_ops, row, &w),
              s2 = agg_expr_eval_i128_as<true, true>(prog, c.n_ops, row, &w);
    if (s0 != AGG_ROW_OVERFLOW || s1 != AGG_ROW_OVERFLOW || s2 != AGG_ROW_OVERFLOW) {
      printf("row %s old-interpreter-gave-a-value %d %d %d\n", name.c_str(), s0, s1, s2);
      return;
    }
  }
  if (st == AGG_ROW_VALUE && c.cls == XCLASS_INT && v != (agg_i128)(long long)v) st = AGG_ROW_OVERFLOW;
  if (st == AGG_ROW_VALUE && c.cls == XCLASS_DEC && (v >= agg_pow10(38) || v <= -agg_pow10(38))) st = AGG_ROW_OVERFLOW;
  printf("row %s %d %s\n", name.c_str(), st, st == AGG_ROW_VALUE ? text_i128(v).c_str() : "0");
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (agg_pow10_38() != agg_pow10(38)) {
    printf("the constant 10^38 is wrong\n");
    return 1;
  }
  std::ifstream in(argv[1]);
  std::string line, prog_name;
  ComputedPlan prog;
  bool have_prog = false;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::vector<std::string> w;
    for (std::string t; ss >> t;) w.push_back(t);
    if (w.empty()) continue;
    if (w[0] == "f" && w.size() >= 3) {
      if (w[1] == "tof64" && w.size() == 4) {
        const uint32_t k = (uint32_t)strtoul(w[3].c_str(), nullptr, 10);
        printf("f %llx\n", agg_bits_of_f64(agg_to_f64(parse_i128(w[2].c_str()), k, agg_pow10(k))));
      } else if (w[1] == "todec" && w.size() == 4) {
        agg_i128 r = 0;
        const bool ok = agg_f64_to_dec(agg_f64_of_bits(strtoull(w[2].c_str(), nullptr, 16)), agg_pow10((uint32_t)strtoul(w[3].c_str(), nullptr, 10)), &r);
        printf("f %d %s\n", (int)ok, text_i128(r).c_str());
      } else if (w[1] == "toi64") {
        agg_i128 r = 0;
        const bool ok = agg_f64_to_i64(agg_f64_of_bits(strtoull(w[2].c_str(), nullptr, 16)), &r);
        printf("f %d %s\n", (int)ok, text_i128(r).c_str());
      } else if (w[1] == "rescale" && w.size() == 5) {
        printf("f %s\n", text_i128(agg_rescale(parse_i128(w[2].c_str()), agg_pow10((uint32_t)strtoul(w[3].c_str(), nullptr, 10)), (uint32_t)strtoul(w[4].c_str(), nullptr, 10))).c_str());
      } else if (w[1] == "fround" && w.size() == 4) {
        printf("f %llx\n", agg_bits_of_f64(agg_f64_round(agg_f64_of_bits(strtoull(w[2].c_str(), nullptr, 16)), (uint32_t)strtoul(w[3].c_str(), nullptr, 10))));
      }
    } else if (w[0] == "plan" && w.size() >= 3) {
      ComputedPlan plan;
      const int rc = compile(std::vector<std::string>(w.begin() + 2, w.end()), plan);
      printf("plan %s %d", w[1].c_str(), rc);
      if (!rc) {
        const ComputedColumn& c = plan.cols[0];
        printf(" %u %d %u", c.cls, c.scale, c.n_ops);
        for (uint32_t k = 0; k < c.n_ops; k++) {
          const AggExprOp& o = plan.ops[c.first_op + k];
          printf(" %u:%u:%llu:%llu", o.op, o.col, o.lo, o.hi);
        }
      }
      printf("\t%s\n", plan.err);
    } else if (w[0] == "pair" && w.size() >= 5) {
      size_t bar = 2;
      while (bar < w.size() && w[bar] != "|") bar++;
      const Expr l = parse(std::vector<std::string>(w.begin() + 2, w.begin() + bar)), r = parse(std::vector<std::string>(w.begin() + (bar < w.size() ? bar + 1 : bar), w.end()));
      const orcgpu_agg_expr lv = l.view(), rv = r.view();
      const std::vector<AggExprCol> xc = columns();
      char err[384] = "";
      AggExprCompiler x{kNames, xc.data(), kN, "a comparison", err, sizeof(err)};
      x.predicate = true;
      AggExprCompiler::Side ls, rs;
      const int rc = x.compile_pair(&lv, &rv, ls, rs);
      printf("pair %s %d %d %d %d %d %d\t%s\n", w[1].c_str(), rc, x.cls, ls.scale, rs.scale, (int)agg_ops_hold_conversion(ls.ops.data(), ls.ops.size()),
             (int)agg_ops_hold_conversion(rs.ops.data(), rs.ops.size()), err);
    } else if (w[0] == "prog" && w.size() >= 3) {
      prog = ComputedPlan();
      prog_name = w[1];
      const int rc = compile(std::vector<std::string>(w.begin() + 2, w.end()), prog);
      have_prog = rc == 0;
      if (rc) printf("prog %s refused %d\t%s\n", w[1].c_str(), rc, prog.err);
    } else if (w[0] == "row" && have_prog) {
      run_row(prog_name, prog, std::vector<std::string>(w.begin() + 1, w.end()));
    }
  }
  return 0;
}
