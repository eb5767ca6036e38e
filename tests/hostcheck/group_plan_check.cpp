// group_plan_check.cpp -- GROUP BY's key compiler, stripe merge and finish step (orc_rust_amd/csrc/orcgpu_group_plan.inc, the very
// text liborcgpu.so is built from) under AddressSanitizer + UBSan, on the CPU (TEST INFRASTRUCTURE).  Reads a file of cases and
// prints what became of each; tests/test_group_plan_sanitized.py holds the lines to the table of include/orcgpu.h.
//   keys <name> <table: flat | nested> <column | -null-> ...   ->  "keys <name> <status> <n> {<kind> <fkind> <scale_or_unit>}\t<message>"
//   stripe <set> <n groups>, then per group "g <count> {key}": one stripe's groups merged into the set <set>; a key is
//        N (NULL) | I<int64> | S<hex bytes, - for none>                 ->  "stripe <set> <status> <groups so far>\t<message>"
//   show <set>                     ->  per group "group <set> <index> <count> {N | I<int64> | S<hex>: what orcgpu_group_key holds}"
//   cap <name> <total groups>      ->  "cap <name> <status> <groups>": stripes of 256 new int keys until <total> were offered
//   flags <name> <flags> <n_groups> ->  "flags <name> <status>\t<message>"
//   mask <name> <env | ->          ->  "mask <name> <hex>"
// The sets' plan is (i64 "i64", string "s").  Exit code 0 when every line was understood; a sanitizer report aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/orcgpu.h"
#include "../../orc_rust_amd/csrc/orcgpu_filter_host.inc"
#include "../../orc_rust_amd/csrc/orcgpu_agg_plan.inc"
#include "../../orc_rust_amd/csrc/orcgpu_group_plan.inc"

using orcgpu_host::AggCol;
using orcgpu_host::GroupPlan;
using orcgpu_host::GroupSet;

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

static int compile(bool nested, const std::vector<const char*>& keys, GroupPlan& plan) {
  const std::vector<Named> t = columns(nested);
  std::vector<const char*> names;
  std::vector<AggCol> cols;
  for (auto& n : t) names.push_back(n.name), cols.push_back(n.col);
  return orcgpu_host::group_compile(keys.empty() ? nullptr : keys.data(), (uint32_t)keys.size(), names.data(), cols.data(), (uint32_t)cols.size(), plan);
}

static std::string unhex(const std::string& h) {
  std::string out;
  for (size_t k = 0; k + 1 < h.size(); k += 2) out.push_back((char)strtoul(h.substr(k, 2).c_str(), nullptr, 16));
  return out;
}

static GroupKeyRecord parse_key(const std::string& tok) {
  GroupKeyRecord r;
  memset(&r, 0, sizeof(r));
  if (tok == "N") {
    r.is_null = 1;
  } else if (tok[0] == 'I') {
    const long long v = strtoll(tok.c_str() + 1, nullptr, 10);
    r.w[0] = (unsigned long long)v;
    r.w[1] = (unsigned long long)(v >> 63);
  } else {
    const std::string b = tok == "S-" ? std::string() : unhex(tok.substr(1));
    r.len = (uint32_t)b.size();
    memcpy(r.bytes, b.data(), b.size() < sizeof(r.bytes) ? b.size() : sizeof(r.bytes));
  }
  return r;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  GroupPlan set_plan;
  {
    std::vector<const char*> keys = {"i64", "s"};
    if (compile(false, keys, set_plan)) return 4;
  }
  std::vector<AggInsn> insns(2);
  insns[0].kind = AK_SUM_INT;
  insns[1].kind = AK_COUNT_ROWS;
  std::map<std::string, GroupSet> sets;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string what, name;
    ss >> what >> name;
    if (what == "keys") {
      std::string table, c;
      ss >> table;
      std::vector<std::string> given;
      while (ss >> c) given.push_back(c);
      std::vector<const char*> keys;
      for (auto& g : given) keys.push_back(g == "-null-" ? nullptr : g.c_str());
      GroupPlan plan;
      const int rc = compile(table == "nested", keys, plan);
      printf("keys %s %d %zu", name.c_str(), rc, plan.keys.size());
      for (auto& k : plan.keys) printf(" %u %u %d", k.kind, k.fkind, k.scale_or_unit);
      printf("\t%s\n", plan.err);
    } else if (what == "stripe") {
      uint32_t n = 0;
      ss >> n;
      std::vector<GroupKeyRecord> keys;
      std::vector<AggPartial> vals;
      for (uint32_t g = 0; g < n; g++) {
        std::getline(in, line);
        std::istringstream gs(line);
        std::string tag, k1, k2;
        long long count = 0;
        gs >> tag >> count >> k1 >> k2;
        keys.push_back(parse_key(k1));
        keys.push_back(parse_key(k2));
        AggPartial sum{}, rows{};
        sum.w[0] = (unsigned long long)count;
        sum.count = 1;
        rows.w[0] = (unsigned long long)count;
        vals.push_back(sum);
        vals.push_back(rows);
      }
      char err[256] = {0};
      const int rc = orcgpu_host::group_merge(set_plan, insns, sets[name], keys.data(), vals.data(), n, err, sizeof(err));
      printf("stripe %s %d %u\t%s\n", name.c_str(), rc, sets[name].n_groups(), err);
    } else if (what == "show") {
      orcgpu_groups out;
      orcgpu_host::group_finish(set_plan, insns, 1, sets[name], out);
      for (uint32_t g = 0; g < out.n_groups; g++) {
        const orcgpu_agg_value& v = out.values[g];
        printf("group %s %u %llu", name.c_str(), g, (unsigned long long)v.w[0]);
        for (uint32_t k = 0; k < out.n_keys; k++) {
          const orcgpu_group_key& key = out.keys[(size_t)g * out.n_keys + k];
          if (key.is_null) {
            printf(" N");
          } else if (key.kind == ORCGPU_GROUP_KEY_STRING) {
            printf(" S");
            for (uint32_t x = 0; x < key.len; x++) printf("%02x", key.bytes[x]);
            if (!key.len) printf("-");
          } else {
            printf(" I%lld", (long long)key.w[0]);
          }
          printf(":%u:%d", key.kind, key.scale_or_unit);
        }
        printf("\n");
      }
    } else if (what == "cap") {
      uint32_t total = 0;
      ss >> total;
      GroupPlan plan;
      std::vector<const char*> keys = {"i32"};
      if (compile(false, keys, plan)) return 4;
      GroupSet set;
      int rc = 0;
      char err[256] = {0};
      for (uint32_t at = 0; at < total && !rc; at += 256) {
        const uint32_t n = total - at < 256 ? total - at : 256;
        std::vector<GroupKeyRecord> recs(n);
        std::vector<AggPartial> vals((size_t)n * 2);
        memset(recs.data(), 0, recs.size() * sizeof(GroupKeyRecord));
        for (uint32_t g = 0; g < n; g++) recs[g].w[0] = at + g;
        rc = orcgpu_host::group_merge(plan, insns, set, recs.data(), vals.data(), n, err, sizeof(err));
      }
      printf("cap %s %d %u\t%s\n", name.c_str(), rc, set.n_groups(), err);
    } else if (what == "flags") {
      uint32_t flags = 0, n = 0;
      ss >> flags >> n;
      const std::vector<Named> t = columns(false);
      std::vector<const char*> names;
      for (auto& c : t) names.push_back(c.name);
      char err[256] = {0};
      const int rc = orcgpu_host::group_check_flags(set_plan, flags, n, names.data(), err, sizeof(err));
      printf("flags %s %d\t%s\n", name.c_str(), rc, err);
    } else if (what == "mask") {
      std::string env;
      ss >> env;
      printf("mask %s %x\n", name.c_str(), orcgpu_host::group_hash_mask(env == "-" ? nullptr : env.c_str()));
    } else if (!what.empty()) {
      fprintf(stderr, "unknown line: %s\n", line.c_str());
      return 3;
    }
  }
  return 0;
}
