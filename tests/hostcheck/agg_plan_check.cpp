// agg_plan_check.cpp -- the aggregation's plan compiler and record arithmetic (orc_rust_amd/csrc/orcgpu_agg_plan.inc, the very text
// liborcgpu.so is built from) under AddressSanitizer + UBSan, on the CPU (TEST INFRASTRUCTURE).  Reads a file of cases and prints
// what became of each; tests/test_agg_plan_sanitized.py holds the lines to the table of include/orcgpu.h and to Python ints.
//   plan <name> <table: flat | nested> <op> <column | -> <column2 | ->   ->  "plan <name> <status> <kind> <is_max> <scale> <fkind>\t<message>"
//   count <name> <n specs>                                               ->  "count <name> <status>"
//   merge <name> <AK kind> <is_max> a0 a1 a2 b0 b1 b2 (hex words)         ->  "merge <name> r0 r1 r2 <fits int128> <fits decimal>"
//   finish <name> <AK kind> <count> <flags> w0 w1 w2                      ->  "finish <name> <value kind> <is_null> <overflow> v0 v1 v2"
// Exit code 0 when every line was understood; a sanitizer report aborts with its own exit code.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/orcgpu.h"
#include "../../orc_rust_amd/csrc/orcgpu_filter_host.inc"
#include "../../orc_rust_amd/csrc/orcgpu_agg_plan.inc"

using orcgpu_host::AggCol;
using orcgpu_host::AggPlan;

struct Named {
  const char* name;
  AggCol col;
};

static AggCol col(int32_t orc_type, uint32_t width, uint32_t scale = 0, int32_t ts_unit = 3, bool dict = false, bool nested = false) {
  AggCol a;
  a.d.orc_type = orc_type;
  a.d.width = width;
  a.d.ts_unit = ts_unit;
  a.d.is_bool = orc_type == ORCGPU_T_BOOLEAN;
  a.d.dict_out = dict;
  a.d.is_string = !dict && (orc_type == ORCGPU_T_STRING || orc_type == ORCGPU_T_BINARY || orc_type == ORCGPU_T_VARCHAR || orc_type == ORCGPU_T_CHAR);
  a.d.has_present = true;
  a.scale = scale;
  a.nested = nested;
  return a;
}

static std::vector<Named> columns(bool nested) {
  std::vector<Named> t = {
      {"i8", col(ORCGPU_T_BYTE, 1)},
      {"i16", col(ORCGPU_T_SHORT, 2)},
      {"i32", col(ORCGPU_T_INT, 4)},
      {"i64", col(ORCGPU_T_LONG, 8)},
      {"date", col(ORCGPU_T_DATE, 4)},
      {"b", col(ORCGPU_T_BOOLEAN, 0)},
      {"f32", col(ORCGPU_T_FLOAT, 4)},
      {"f64", col(ORCGPU_T_DOUBLE, 8)},
      {"dec15_2", col(ORCGPU_T_DECIMAL, 16, 2)},
      {"dec38_0", col(ORCGPU_T_DECIMAL, 16, 0)},
      {"dec38_19", col(ORCGPU_T_DECIMAL, 16, 19)},
      {"dec38_20", col(ORCGPU_T_DECIMAL, 16, 20)},
      {"ts", col(ORCGPU_T_TIMESTAMP, 8, 0, 3)},
      {"ts_us", col(ORCGPU_T_TIMESTAMP, 8, 0, 2)},
      {"tsi", col(ORCGPU_T_TIMESTAMP_INSTANT, 8, 0, 3)},
      {"ts9", col(ORCGPU_T_TIMESTAMP, 16, 0, 4)},
      {"s", col(ORCGPU_T_STRING, 0)},
      {"bin", col(ORCGPU_T_BINARY, 0)},
      {"vc", col(ORCGPU_T_VARCHAR, 0)},
      {"ch", col(ORCGPU_T_CHAR, 0)},
      {"dict", col(ORCGPU_T_STRING, 4, 0, 3, true)},
      {"i64_as_i16", col(ORCGPU_T_LONG, 2)},
  };
  if (nested) t.push_back({"st", col(ORCGPU_T_STRUCT, 0, 0, 3, false, true)});
  return t;
}

static unsigned long long hex(const std::string& s) { return strtoull(s.c_str(), nullptr, 16); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string what, name;
    ss >> what >> name;
    if (what == "plan") {
      std::string table, c1, c2;
      uint32_t op = 0;
      ss >> table >> op >> c1 >> c2;
      const std::vector<Named> t = columns(table == "nested");
      std::vector<const char*> names;
      std::vector<AggCol> cols;
      for (auto& n : t) names.push_back(n.name), cols.push_back(n.col);
      orcgpu_agg_spec spec{op, c1 == "-" ? nullptr : c1.c_str(), c2 == "-" ? nullptr : c2.c_str()};
      AggPlan plan;
      const int rc = orcgpu_host::agg_compile(&spec, 1, names.data(), cols.data(), (uint32_t)cols.size(), plan);
      if (rc || plan.insns.size() != 1) printf("plan %s %d 0 0 0 0\t%s\n", name.c_str(), rc ? rc : -1, plan.err);
      else printf("plan %s 0 %u %u %d %u\t\n", name.c_str(), plan.insns[0].kind, plan.insns[0].is_max, plan.insns[0].scale, plan.insns[0].fkind);
    } else if (what == "count") {
      uint32_t n = 0;
      ss >> n;
      const std::vector<Named> t = columns(false);
      std::vector<const char*> names;
      std::vector<AggCol> cols;
      for (auto& c : t) names.push_back(c.name), cols.push_back(c.col);
      std::vector<orcgpu_agg_spec> specs(n, orcgpu_agg_spec{ORCGPU_AGG_OP_COUNT_ROWS, nullptr, nullptr});
      AggPlan plan;
      const int rc = orcgpu_host::agg_compile(specs.data(), n, names.data(), cols.data(), (uint32_t)cols.size(), plan);
      printf("count %s %d %zu\n", name.c_str(), rc, plan.insns.size());
    } else if (what == "merge") {
      AggInsn insn{};
      std::string w[6];
      ss >> insn.kind >> insn.is_max;
      for (auto& x : w) ss >> x;
      AggPartial a{}, b{};
      for (int k = 0; k < 3; k++) a.w[k] = hex(w[k]), b.w[k] = hex(w[3 + k]);
      a.count = b.count = 1;
      orcgpu_host::agg_merge(insn, a, b);
      printf("merge %s %llx %llx %llx %d %d\n", name.c_str(), a.w[0], a.w[1], a.w[2], (int)orcgpu_host::agg_fits_i128(a.w), (int)orcgpu_host::agg_fits_decimal(a.w));
    } else if (what == "finish") {
      AggInsn insn{};
      AggPartial p{};
      std::string w[3];
      ss >> insn.kind >> p.count >> p.flags >> w[0] >> w[1] >> w[2];
      for (int k = 0; k < 3; k++) p.w[k] = hex(w[k]);
      insn.scale = 7;
      orcgpu_agg_value v;
      orcgpu_host::agg_finish(insn, p, &v);
      printf("finish %s %u %u %u %llx %llx %llx %d\n", name.c_str(), v.kind, v.is_null, v.overflow, (unsigned long long)v.w[0], (unsigned long long)v.w[1],
             (unsigned long long)v.w[2], v.f != v.f);
    } else if (!what.empty()) {
      fprintf(stderr, "unknown line: %s\n", line.c_str());
      return 3;
    }
  }
  return 0;
}
