// agg_expr_check.cpp -- the expression aggregates' plan compiler (orc_rust_amd/csrc/orcgpu_agg_expr.inc), the evaluator the kernels
// run (orc_rust_amd/csrc/device/agg_expr_eval.h) and AVG's division (orcgpu_agg_plan.inc: agg_finish), the very text liborcgpu.so is
// built from, under AddressSanitizer + UBSan on the CPU (TEST INFRASTRUCTURE).  Reads a file of cases and prints what became of each;
// tests/test_agg_expr_plan_sanitized.py holds the lines to include/orcgpu.h and to Python ints, Fractions and Decimals.
//
// An expression is written in pre-order, one token a node: c:<column>  i:<int64>  f:<double as %a or decimal>  d:<unscaled>:<scale>
// + - * neg, and for the malformed ones x:<node op>  v:<value type> (a literal of that type)  dbad:<s_len>:<scale> (a bad Decimal).
//   plan <name> <op> <tokens...>                      -> "plan <name> <status> <kind> <scale> <n ops> <max slots>\t<message>"
//   eval <name> <tokens...> | <column>=<value|null>.. -> "eval <name> <status> <row: 0 null, 1 value, 2 overflow> <value: int or %a>"
//   arith <name> <add|sub|mul|neg|scale> <a> <b>       -> "arith <name> <fits> <result>"
//   avg <name> <AK kind> <scale> <count> <flags> <sum> -> "avg <name> <value kind> <is_null> <overflow> <scale> <int of w, or %a of f>"
// Exit code 0 when every line was understood; a sanitizer report aborts with its own exit code.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/orcgpu.h"
#include "../../orc_rust_amd/csrc/orcgpu_filter_host.inc"
#include "../../orc_rust_amd/csrc/orcgpu_agg_plan.inc"

using orcgpu_host::AggCol;
using orcgpu_host::AggPlan;

static AggCol col(int32_t orc_type, uint32_t width, uint32_t scale = 0, int32_t ts_unit = 3, bool dict = false) {
  AggCol a;
  a.d.orc_type = orc_type;
  a.d.width = width;
  a.d.ts_unit = ts_unit;
  a.d.is_bool = orc_type == ORCGPU_T_BOOLEAN;
  a.d.dict_out = dict;
  a.d.is_string = !dict && (orc_type == ORCGPU_T_STRING || orc_type == ORCGPU_T_BINARY);
  a.d.has_present = true;
  a.scale = scale;
  return a;
}
struct Named {
  const char* name;
  AggCol col;
};
static const std::vector<Named>& columns() {
  static const std::vector<Named> t = {
      {"i8", col(ORCGPU_T_BYTE, 1)},          {"i16", col(ORCGPU_T_SHORT, 2)},          {"i32", col(ORCGPU_T_INT, 4)},
      {"i64", col(ORCGPU_T_LONG, 8)},         {"j64", col(ORCGPU_T_LONG, 8)},           {"k64", col(ORCGPU_T_LONG, 8)},
      {"f32", col(ORCGPU_T_FLOAT, 4)},        {"f64", col(ORCGPU_T_DOUBLE, 8)},         {"g64", col(ORCGPU_T_DOUBLE, 8)},
      {"dec15_2", col(ORCGPU_T_DECIMAL, 16, 2)}, {"dec12_5", col(ORCGPU_T_DECIMAL, 16, 5)}, {"dec38_0", col(ORCGPU_T_DECIMAL, 16, 0)},
      {"dec38_19", col(ORCGPU_T_DECIMAL, 16, 19)}, {"dec38_20", col(ORCGPU_T_DECIMAL, 16, 20)}, {"dec38_38", col(ORCGPU_T_DECIMAL, 16, 38)},
      {"date", col(ORCGPU_T_DATE, 4)},        {"b", col(ORCGPU_T_BOOLEAN, 0)},          {"ts", col(ORCGPU_T_TIMESTAMP, 8, 0, 3)},
      {"ts9", col(ORCGPU_T_TIMESTAMP, 16, 0, 4)}, {"s", col(ORCGPU_T_STRING, 0)},       {"dict", col(ORCGPU_T_STRING, 4, 0, 3, true)},
      {"i64_as_i16", col(ORCGPU_T_LONG, 2)},
  };
  return t;
}

static agg_i128 parse_i128(const std::string& s) {
  size_t k = 0;
  bool neg = false;
  if (k < s.size() && s[k] == '-') neg = true, k++;
  agg_u128 v = 0;
  for (; k < s.size(); k++) v = v * 10 + (agg_u128)(s[k] - '0');
  return (agg_i128)(neg ? (agg_u128)0 - v : v);
}
static std::string str_i128(agg_i128 x) {
  const bool neg = x < 0;
  agg_u128 v = neg ? (agg_u128)0 - (agg_u128)x : (agg_u128)x;
  std::string s;
  do {
    s.insert(s.begin(), (char)('0' + (int)(v % 10)));
    v /= 10;
  } while (v);
  return neg ? "-" + s : s;
}
// a signed 192-bit integer as decimal: the words little-endian
static std::string str_i192(const unsigned long long* w) {
  unsigned long long m[3];
  const bool neg = agg_abs192(w, m);
  std::string s;
  do {
    const unsigned long long r = agg_div192_u64(m, 10);
    s.insert(s.begin(), (char)('0' + (int)r));
  } while (m[0] || m[1] || m[2]);
  return neg ? "-" + s : s;
}
static void words_of(const std::string& s, unsigned long long* w) {  // a decimal string of up to 192 bits
  size_t k = 0;
  bool neg = false;
  if (k < s.size() && s[k] == '-') neg = true, k++;
  unsigned long long m[3] = {0, 0, 0};
  for (; k < s.size(); k++) {
    agg_mul192_u64(m, 10);
    unsigned long long add = (unsigned long long)(s[k] - '0');
    for (int x = 0; x < 3 && add; x++) {
      m[x] += add;
      add = m[x] < add ? 1 : 0;
    }
  }
  unsigned long long carry = neg ? 1 : 0;
  for (int x = 0; x < 3; x++) {
    const unsigned long long v = neg ? ~m[x] : m[x];
    w[x] = v + carry;
    carry = carry && w[x] == 0;
  }
}

struct Tokens {
  std::vector<orcgpu_agg_expr_node> nodes;
  std::vector<std::string> keep;  // (reserved up front: the nodes point into it)
  Tokens() { keep.reserve(256); }
  bool add(const std::string& tok) {
    orcgpu_agg_expr_node n{};
    const std::string arg = tok.size() > 2 ? tok.substr(tok.find(':') + 1) : "";
    if (tok == "+") n.op = ORCGPU_AGG_EXPR_ADD;
    else if (tok == "-") n.op = ORCGPU_AGG_EXPR_SUB;
    else if (tok == "*") n.op = ORCGPU_AGG_EXPR_MUL;
    else if (tok == "neg") n.op = ORCGPU_AGG_EXPR_NEG;
    else if (tok.rfind("c:", 0) == 0) {
      n.op = ORCGPU_AGG_EXPR_COLUMN;
      if (arg != "NULL") {
        keep.push_back(arg);
        n.column = keep.back().c_str();
      }
    } else if (tok.rfind("i:", 0) == 0) {
      n.op = ORCGPU_AGG_EXPR_LITERAL;
      n.value_type = ORCGPU_PV_INT64;
      n.i = (int64_t)parse_i128(arg);
    } else if (tok.rfind("f:", 0) == 0) {
      n.op = ORCGPU_AGG_EXPR_LITERAL;
      n.value_type = ORCGPU_PV_FLOAT64;
      n.f = strtod(arg.c_str(), nullptr);
    } else if (tok.rfind("d:", 0) == 0) {
      n.op = ORCGPU_AGG_EXPR_LITERAL;
      n.value_type = ORCGPU_PV_DECIMAL128;
      const size_t c = arg.find(':');
      const agg_i128 v = parse_i128(arg.substr(0, c));
      std::string bytes(16, '\0');
      for (int k = 0; k < 16; k++) bytes[k] = (char)(uint8_t)((agg_u128)v >> (8 * k));
      keep.push_back(bytes);
      n.s = keep.back().data();
      n.s_len = 16;
      n.i = atoll(arg.substr(c + 1).c_str());
    } else if (tok.rfind("dbad:", 0) == 0) {
      n.op = ORCGPU_AGG_EXPR_LITERAL;
      n.value_type = ORCGPU_PV_DECIMAL128;
      const size_t c = arg.find(':');
      keep.push_back(std::string(32, '\x7f'));  // (16 bytes of 0x7f: a magnitude past 10^38)
      n.s = keep.back().data();
      n.s_len = (uint64_t)atoll(arg.substr(0, c).c_str());
      n.i = atoll(arg.substr(c + 1).c_str());
    } else if (tok.rfind("x:", 0) == 0) {
      n.op = (uint32_t)strtoul(arg.c_str(), nullptr, 10);
    } else if (tok.rfind("v:", 0) == 0) {
      n.op = ORCGPU_AGG_EXPR_LITERAL;
      n.value_type = atoi(arg.c_str());
      n.i = 1;
      n.f = 1.0;
    } else {
      return false;
    }
    nodes.push_back(n);
    return true;
  }
};

struct HostRow {
  std::vector<bool> ok;
  std::vector<agg_i128> iv;
  std::vector<double> fv;
  bool valid(uint32_t c) const { return ok[c]; }
  agg_i128 load_int(uint32_t c) const { return iv[c]; }
  agg_i128 load_dec(uint32_t c) const { return iv[c]; }
  double load_f64(uint32_t c) const { return fv[c]; }
};

// the largest number of operand slots in use while the program runs, and whether every op finds its operands
static int max_slots(const std::vector<AggExprOp>& ops) {
  int depth = 0, most = 0;
  for (const AggExprOp& o : ops) {
    if (o.op >= AX_PUSH_INT && o.op <= AX_PUSH_LIT) depth++;
    else if (o.op >= AX_ADD && o.op <= AX_MUL) {
      if (depth < 2) return -1;
      depth--;
    } else if ((o.op == AX_NEG || o.op == AX_SCALE10) && depth < 1) return -1;
    most = depth > most ? depth : most;
  }
  return depth == 1 ? most : -1;
}

static int compile(const Tokens& t, uint32_t op, AggPlan& plan, bool no_expr = false) {
  std::vector<const char*> names;
  std::vector<AggCol> cols;
  for (auto& n : columns()) names.push_back(n.name), cols.push_back(n.col);
  orcgpu_agg_spec spec{op, nullptr, nullptr};
  orcgpu_agg_expr e{t.nodes.data(), (uint32_t)t.nodes.size()};
  return orcgpu_host::agg_compile(&spec, no_expr ? nullptr : &e, 1, names.data(), cols.data(), (uint32_t)cols.size(), plan);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string what, name, tok;
    ss >> what >> name;
    if (what == "plan") {
      uint32_t op = 0;
      ss >> op;
      Tokens t;
      bool none = false;
      while (ss >> tok) {
        if (tok == "none") none = true;
        else if (!t.add(tok)) return 3;
      }
      AggPlan plan;
      const int rc = compile(t, op, plan, none);
      if (rc || plan.insns.size() != 1) printf("plan %s %d 0 0 0 0\t%s\n", name.c_str(), rc ? rc : -1, plan.err);
      else printf("plan %s 0 %u %d %zu %d\t\n", name.c_str(), plan.insns[0].kind, plan.insns[0].scale, plan.ops.size(), max_slots(plan.ops));
    } else if (what == "eval") {
      Tokens t;
      while (ss >> tok && tok != "|")
        if (!t.add(tok)) return 3;
      HostRow row;
      row.ok.assign(columns().size(), true);
      row.iv.assign(columns().size(), 0);
      row.fv.assign(columns().size(), 0.0);
      while (ss >> tok) {
        const size_t eq = tok.find('=');
        const std::string cname = tok.substr(0, eq), val = tok.substr(eq + 1);
        for (size_t c = 0; c < columns().size(); c++) {
          if (cname != columns()[c].name) continue;
          if (val == "null") row.ok[c] = false;
          else if (columns()[c].col.d.orc_type == ORCGPU_T_FLOAT || columns()[c].col.d.orc_type == ORCGPU_T_DOUBLE) row.fv[c] = strtod(val.c_str(), nullptr);
          else row.iv[c] = parse_i128(val);
        }
      }
      AggPlan plan;
      const int rc = compile(t, ORCGPU_AGG_OP_SUM_EXPR, plan);
      if (rc) {
        printf("eval %s %d 0 0\n", name.c_str(), rc);
        continue;
      }
      const AggInsn& insn = plan.insns[0];
      if (max_slots(plan.ops) < 1 || max_slots(plan.ops) > (int)kAggExprSlots || insn.col + insn.col2 != plan.ops.size()) return 4;
      if (insn.kind == AK_EXPR_F64) {
        double v = 0;
        const int r = agg_expr_eval_f64(plan.ops.data() + insn.col, insn.col2, row, &v);
        printf("eval %s 0 %d %a\n", name.c_str(), r, r == AGG_ROW_VALUE ? v : 0.0);
      } else {
        agg_i128 v = 0;
        const int r = agg_expr_eval_i128(plan.ops.data() + insn.col, insn.col2, row, &v);
        printf("eval %s 0 %d %s\n", name.c_str(), r, r == AGG_ROW_VALUE ? str_i128(v).c_str() : "0");
      }
    } else if (what == "arith") {
      std::string op, a, b;
      ss >> op >> a >> b;
      const agg_i128 x = parse_i128(a), y = parse_i128(b);
      agg_i128 r = 0;
      const bool ok = op == "add" ? agg_add_checked(x, y, &r) : op == "sub" ? agg_sub_checked(x, y, &r) : op == "mul" ? agg_mul_checked(x, y, &r)
                    : op == "neg" ? agg_neg_checked(x, &r) : agg_mul_checked(x, agg_pow10((uint32_t)y), &r);
      printf("arith %s %d %s\n", name.c_str(), (int)ok, ok ? str_i128(r).c_str() : "0");
    } else if (what == "avg") {
      AggInsn insn{};
      AggPartial p{};
      std::string sum;
      ss >> insn.kind >> insn.scale >> p.count >> p.flags >> sum;
      insn.op = ORCGPU_AGG_OP_AVG;
      if (insn.kind == AK_SUM_F64) p.f = strtod(sum.c_str(), nullptr);
      else words_of(sum, p.w);
      orcgpu_agg_value v;
      orcgpu_host::agg_finish(insn, p, &v);
      if (v.kind == ORCGPU_AGG_KIND_F64) printf("avg %s %u %u %u %d %a\n", name.c_str(), v.kind, v.is_null, v.overflow, v.scale_or_unit, v.f);
      else {
        unsigned long long w[3] = {v.w[0], v.w[1], v.w[2]};
        printf("avg %s %u %u %u %d %s\n", name.c_str(), v.kind, v.is_null, v.overflow, v.scale_or_unit, str_i192(w).c_str());
      }
    } else if (!what.empty()) {
      fprintf(stderr, "unknown line: %s\n", line.c_str());
      return 3;
    }
  }
  return 0;
}
