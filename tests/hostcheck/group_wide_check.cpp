// group_wide_check.cpp -- the host side of GROUP BY's limits and wide path (orc_rust_amd/csrc/orcgpu_group_plan.inc, the very text
// liborcgpu.so is built from) under AddressSanitizer + UBSan, on the CPU (TEST INFRASTRUCTURE).  Reads a file of cases and prints
// what became of each; tests/test_group_wide_plan_sanitized.py holds the lines to what include/orcgpu.h and INTEGRATION.md 6g say.
//   limits <name> <max_groups> <max_total>            ->  "limits <name> <status> <max_groups> <max_total>\t<message>"
//   plan <limit>                                      ->  "plan <limit> <wide 0 / 1> <slots> <passes>"
//   layout <limit> <n_in> <n_insn> <n_keys> <base>    ->  "layout <limit> <n_in> <n_insn> <n_keys> <slots> <passes> <tiles> <cap> <bytes> {<table>:<offset>:<size>}"
//   merge <name> <max_total> <stripes> <per> <step>   ->  stripe s offers the int keys s * step .. s * step + per - 1, key k with the
//        sum k + s and one row:  "merge <name> <status> <groups>\t<message>", then per group "mgroup <name> <index> <key> <sum> <rows>"
//   flags <name> <max_groups> <flags> <n_groups>      ->  "flags <name> <status>\t<message>"
// Exit code 0 when every line was understood; a sanitizer report aborts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
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
using orcgpu_host::GroupWideLayout;

static GroupPlan int_plan() {
  AggCol c;
  c.d.orc_type = ORCGPU_T_LONG;
  c.d.width = 8;
  c.d.has_present = true;
  const char* names[1] = {"k"};
  GroupPlan plan;
  if (orcgpu_host::group_compile(names, 1, names, &c, 1, plan)) exit(4);
  return plan;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string what;
    ss >> what;
    if (what == "limits") {
      std::string name;
      uint32_t g = 0, t = 0, og = 0, ot = 0;
      ss >> name >> g >> t;
      char err[256] = {0};
      const int rc = orcgpu_host::group_limits(g, t, &og, &ot, err, sizeof(err));
      printf("limits %s %d %u %u\t%s\n", name.c_str(), rc, og, ot, err);
    } else if (what == "plan") {
      uint32_t limit = 0;
      ss >> limit;
      printf("plan %u %d %u %u\n", limit, orcgpu_host::group_is_wide(limit) ? 1 : 0, orcgpu_host::group_wide_slots(limit), orcgpu_host::group_wide_passes(limit));
    } else if (what == "layout") {
      uint32_t limit = 0, n_insn = 0, n_keys = 0;
      uint64_t n_in = 0, base = 0;
      ss >> limit >> n_in >> n_insn >> n_keys >> base;
      const GroupWideLayout w = orcgpu_host::group_wide_layout(base, limit, n_in, n_insn, n_keys);
      const uint64_t padded = (n_in + 63) / 64 * 64;
      printf("layout %u %llu %u %u %u %u %u %u %llu", limit, (unsigned long long)n_in, n_insn, n_keys, w.slots, w.passes, w.tiles, w.cap, (unsigned long long)w.bytes);
      const struct {
        const char* name;
        uint64_t off, size;
      } parts[] = {{"table", w.o_table, w.table_bytes},
                   {"plane", w.o_plane, padded * 4},
                   {"slot_group", w.o_slot_group, (uint64_t)w.slots * 4},
                   {"blk_first", w.o_blk_first, (uint64_t)w.tiles * 4},
                   {"blk_kept", w.o_blk_kept, (uint64_t)w.tiles * 4},
                   {"keys0", w.o_keys[0], padded * 4},
                   {"keys1", w.o_keys[1], padded * 4},
                   {"rows0", w.o_rows[0], padded * 4},
                   {"rows1", w.o_rows[1], padded * 4},
                   {"hist", w.o_hist, (uint64_t)w.tiles * 256 * 4},
                   {"seg", w.o_seg, (uint64_t)w.cap * 4},
                   {"ctl", w.o_ctl, sizeof(GroupControl)},
                   {"key_recs", w.o_key_recs, (uint64_t)w.cap * n_keys * sizeof(GroupKeyRecord)},
                   {"vals", w.o_vals, (uint64_t)w.cap * n_insn * sizeof(AggPartial)}};
      for (auto& p : parts) printf(" %s:%llu:%llu", p.name, (unsigned long long)p.off, (unsigned long long)p.size);
      printf("\n");
    } else if (what == "merge") {
      std::string name;
      uint32_t max_total = 0, stripes = 0, per = 0, step = 0;
      ss >> name >> max_total >> stripes >> per >> step;
      GroupPlan plan = int_plan();
      plan.max_groups = per;
      plan.max_total = max_total;
      std::vector<AggInsn> insns(2);
      insns[0].kind = AK_SUM_INT;
      insns[1].kind = AK_COUNT_ROWS;
      GroupSet set;
      int rc = 0;
      char err[256] = {0};
      for (uint32_t s = 0; s < stripes && !rc; s++) {
        std::vector<GroupKeyRecord> recs(per);
        std::vector<AggPartial> vals((size_t)per * 2);
        memset(recs.data(), 0, recs.size() * sizeof(GroupKeyRecord));
        for (uint32_t g = 0; g < per; g++) {
          recs[g].w[0] = (uint64_t)s * step + g;
          vals[(size_t)g * 2].w[0] = (uint64_t)s * step + g + s;
          vals[(size_t)g * 2].count = 1;
          vals[(size_t)g * 2 + 1].w[0] = 1;
        }
        rc = orcgpu_host::group_merge(plan, insns, set, recs.data(), vals.data(), per, err, sizeof(err));
      }
      printf("merge %s %d %u\t%s\n", name.c_str(), rc, set.n_groups(), err);
      if (!rc) {
        orcgpu_groups out;
        orcgpu_host::group_finish(plan, insns, 1, set, out);
        for (uint32_t g = 0; g < out.n_groups; g++)
          printf("mgroup %s %u %lld %lld %llu\n", name.c_str(), g, (long long)out.keys[g].w[0], (long long)out.values[g].w[0], (unsigned long long)set.vals[(size_t)g * 2 + 1].w[0]);
      }
    } else if (what == "flags") {
      std::string name;
      uint32_t max_groups = 0, flags = 0, n = 0;
      ss >> name >> max_groups >> flags >> n;
      GroupPlan plan = int_plan();
      plan.max_groups = max_groups;
      const char* names[1] = {"k"};
      char err[256] = {0};
      const int rc = orcgpu_host::group_check_flags(plan, flags, n, names, err, sizeof(err));
      printf("flags %s %d\t%s\n", name.c_str(), rc, err);
    } else if (!what.empty()) {
      fprintf(stderr, "unknown line: %s\n", line.c_str());
      return 3;
    }
  }
  return 0;
}
