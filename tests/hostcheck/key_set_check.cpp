// key_set_check.cpp -- the host side of the key sets (orc_rust_amd/csrc/orcgpu_key_set.inc, the set leaf of orcgpu_filter_plan.inc
// and the probe of device/filter_program.h, the very text liborcgpu.so is built from) under AddressSanitizer + UBSan, on the CPU
// (TEST INFRASTRUCTURE).  A stand-alone program: it builds its cases itself and prints one line per fact,
// "<name> <values ...>[\t<message>]"; tests/test_key_set_host_sanitized.py holds the lines to what include/orcgpu.h says.  Exit
// code 0 when it ran through; a sanitizer report aborts with its own exit code.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/orcgpu.h"
#include "../../orc_rust_amd/csrc/orcgpu_filter_plan.inc"

using namespace orcgpu_host;

static void show_layout(const char* name, uint64_t max_keys) {
  KeySetLayout lay;
  const bool ok = key_set_layout(max_keys, lay);
  printf("%s %d %u %llu %llu %llu %llu\n", name, ok ? 1 : 0, lay.n_slots, (unsigned long long)lay.o_occ, (unsigned long long)lay.o_slots,
         (unsigned long long)lay.table_bytes, (unsigned long long)lay.bytes);
}

// A sealed table of `keys` built on the host; every key present, every one of `absent` absent, by in_table / in_probe_i64
static void show_probe(const char* name, const std::vector<uint64_t>& keys, const std::vector<uint64_t>& absent, uint64_t max_keys, uint32_t hash_mask) {
  std::vector<uint8_t> tab;
  const bool built = key_set_build_host(keys.data(), keys.size(), false, max_keys, hash_mask, tab);
  // (the probe reads 8-byte words: the bytes go to an aligned home)
  std::vector<uint64_t> home((tab.size() + 7) / 8);
  if (!tab.empty()) memcpy(home.data(), tab.data(), tab.size());
  const InTable t = in_table(reinterpret_cast<const uint8_t*>(home.data()), (uint32_t)tab.size());
  size_t found = 0, wrong = 0, longest = 0;
  for (uint64_t k : keys) found += t.n_slots && in_probe_i64(t, k);
  for (uint64_t k : absent) wrong += t.n_slots && in_probe_i64(t, k);
  // the longest run of occupied slots, wrapping round: how long a chain can be
  for (uint32_t s = 0, run = 0; t.n_slots && s < 2 * t.n_slots; s++) {
    run = ((t.occ[(s & (t.n_slots - 1)) >> 6] >> (s & 63)) & 1) ? run + 1 : 0;
    if (run > longest) longest = run;
  }
  const uint32_t* h = reinterpret_cast<const uint32_t*>(home.data());
  printf("%s %d %u %zu %zu %zu %u %u %u %u\n", name, built ? 1 : 0, t.n_slots, found, wrong, longest, built ? h[0] : 0, built ? h[2] : 0, built ? h[5] : 0, built ? ~h[6] : 0);
}

static const char* const kNames[] = {"i8", "i16", "i32", "i64", "date", "ts", "dec", "f64", "b", "s", "tsi"};
static const int32_t kKinds[] = {ORCGPU_T_BYTE, ORCGPU_T_SHORT, ORCGPU_T_INT, ORCGPU_T_LONG, ORCGPU_T_DATE, ORCGPU_T_TIMESTAMP, ORCGPU_T_DECIMAL, ORCGPU_T_DOUBLE,
                                 ORCGPU_T_BOOLEAN, ORCGPU_T_STRING, ORCGPU_T_TIMESTAMP_INSTANT};
static const uint32_t kNc = 11;

static orcgpu_predicate_node leaf(int32_t op, const char* column, int64_t i = 0, uint32_t kids = 0) {
  orcgpu_predicate_node n;
  memset(&n, 0, sizeof(n));
  n.op = op;
  n.column = column;
  n.i = i;
  n.n_children = kids;
  return n;
}
static orcgpu_predicate_node int_lit(int32_t op, const char* column, int64_t v) {
  orcgpu_predicate_node n = leaf(op, column, v);
  n.value_type = ORCGPU_PV_INT64;
  return n;
}

static KeySetRefs the_sets(std::shared_ptr<void> hold) {
  KeySetRefs sets(5);
  sets[0].id = 7, sets[0].state = KEY_SET_SEALED, sets[0].table = 0x7f0000001000ull, sets[0].bytes = 32 + 8 + 64 * 8, sets[0].n_keys = 20, sets[0].max_keys = 32;
  sets[1] = sets[0], sets[1].id = 8, sets[1].has_null = true, sets[1].table = 0x7f0000002000ull;
  sets[2].id = 9, sets[2].state = KEY_SET_BUILDING, sets[2].max_keys = 32;
  sets[3].id = 10, sets[3].state = KEY_SET_FAILED, sets[3].max_keys = 32;
  sets[4].id = 11, sets[4].state = KEY_SET_SEALED, sets[4].max_keys = 32;  // (sealed, and empty)
  for (auto& s : sets) s.hold = hold;
  return sets;
}

// rc, then per instruction op:cmp:col:i:lo:lit_off:lit_len, then the IN leaves' list and the holds
static void show_compile(const char* name, const std::vector<orcgpu_predicate_node>& nodes, const KeySetRefs* sets) {
  FilterPlan plan;
  const int rc = filter_compile(nodes.data(), (uint32_t)nodes.size(), kNames, kKinds, kNc, plan, nullptr, sets);
  printf("%s %d", name, rc);
  if (!rc) {
    for (const FilterInsn& in : plan.prog)
      printf(" %u:%u:%u:%lld:%llu:%llu:%u", in.op, in.cmp, in.col, in.i, in.lo, in.op == FOP_IN_SET ? in.lit_off : 0ull, in.op == FOP_IN_SET ? in.lit_len : 0u);
    printf(" leaves=%zu planes=%zu holds=%zu", plan.in_leaves.size(), plan.n_planes(), plan.holds.size());
  }
  printf("\t%s\n", plan.err);
}

int main() {
  // ---- slot count and byte size per max_keys ----
  show_layout("lay_1", 1);
  show_layout("lay_32", 32);
  show_layout("lay_33", 33);
  show_layout("lay_max", 1ull << 26);
  show_layout("lay_0", 0);
  show_layout("lay_over", (1ull << 26) + 1);
  printf("mask %u %u %u %u %u %u\n", key_set_hash_mask(nullptr), key_set_hash_mask(""), key_set_hash_mask("1"), key_set_hash_mask("4"), key_set_hash_mask("32"),
         key_set_hash_mask("0"));

  // ---- a sealed table on the host answers the probe ----
  std::vector<uint64_t> keys, absent;
  for (uint64_t k = 0; k < 300; k++) keys.push_back(k * 7919 - 1000), absent.push_back(k * 7919 - 1000 + 1);
  show_probe("probe_300", keys, absent, 1024, 0xffffffffu);
  show_probe("probe_300_bits1", keys, absent, 1024, 1u);
  show_probe("probe_300_bits4", keys, absent, 1024, 15u);
  const std::vector<uint64_t> edge = {0x8000000000000000ull, 0x7fffffffffffffffull, 0, ~0ull, kKeySetFree};
  show_probe("probe_edge", edge, {1, 2, kKeySetFree + 1, 0x8000000000000001ull}, 32, 0xffffffffu);
  show_probe("probe_full_32", std::vector<uint64_t>(keys.begin(), keys.begin() + 32), absent, 32, 0xffffffffu);
  show_probe("probe_33_of_32", std::vector<uint64_t>(keys.begin(), keys.begin() + 33), absent, 32, 0xffffffffu);
  show_probe("probe_none", {}, absent, 32, 0xffffffffu);

  // ---- op 26 -> FOP_IN_SET ----
  auto hold = std::make_shared<int>(0);
  {
    const KeySetRefs sets = the_sets(hold);
    show_compile("set_i64", {leaf(ORCGPU_PRED_IN_SET, "i64", 7)}, &sets);
    show_compile("set_null_date", {leaf(ORCGPU_PRED_IN_SET, "date", 8)}, &sets);
    show_compile("set_i8", {leaf(ORCGPU_PRED_IN_SET, "i8", 7)}, &sets);
    show_compile("set_empty", {leaf(ORCGPU_PRED_IN_SET, "i32", 11)}, &sets);
    // planes are numbered with the IN leaves': IN list (plane 0), set (1), NOT set (2)
    std::vector<orcgpu_predicate_node> mix = {leaf(ORCGPU_PRED_AND, nullptr, 0, 3), leaf(ORCGPU_PRED_IN, "i32", 0, 2), int_lit(ORCGPU_PRED_LITERAL, nullptr, 4),
                                              int_lit(ORCGPU_PRED_LITERAL, nullptr, 5), leaf(ORCGPU_PRED_IN_SET, "i64", 7), leaf(ORCGPU_PRED_NOT, nullptr, 0, 1),
                                              leaf(ORCGPU_PRED_IN_SET, "i16", 8)};
    show_compile("mix", mix, &sets);
    printf("hold_uses %ld\n", hold.use_count());
    // append: a condition's plan behind a row filter's -- the table's address stays, the plane moves
    FilterPlan a, b;
    const std::vector<orcgpu_predicate_node> n1 = {leaf(ORCGPU_PRED_IN, "i32", 0, 2), int_lit(ORCGPU_PRED_LITERAL, nullptr, 4), int_lit(ORCGPU_PRED_LITERAL, nullptr, 5)};
    const std::vector<orcgpu_predicate_node> n2 = {leaf(ORCGPU_PRED_IN_SET, "i64", 7)};
    filter_compile(n1.data(), 3, kNames, kKinds, kNc, a, nullptr, &sets);
    filter_compile(n2.data(), 1, kNames, kKinds, kNc, b, nullptr, &sets);
    const uint32_t first = filter_plan_append(a, b);
    const FilterInsn& in = a.prog[first];
    printf("append %u %u %lld %llu %u %zu %zu\n", first, in.op, in.i, in.lit_off, in.lit_len, a.in_leaves.size(), a.holds.size());
    // ---- the refusals ----
    show_compile("ref_ts", {leaf(ORCGPU_PRED_IN_SET, "ts", 7)}, &sets);
    show_compile("ref_tsi", {leaf(ORCGPU_PRED_IN_SET, "tsi", 7)}, &sets);
    show_compile("ref_dec", {leaf(ORCGPU_PRED_IN_SET, "dec", 7)}, &sets);
    show_compile("ref_f64", {leaf(ORCGPU_PRED_IN_SET, "f64", 7)}, &sets);
    show_compile("ref_bool", {leaf(ORCGPU_PRED_IN_SET, "b", 7)}, &sets);
    show_compile("ref_string", {leaf(ORCGPU_PRED_IN_SET, "s", 7)}, &sets);
    show_compile("ref_unknown_column", {leaf(ORCGPU_PRED_IN_SET, "nope", 7)}, &sets);
    show_compile("ref_no_column", {leaf(ORCGPU_PRED_IN_SET, nullptr, 7)}, &sets);
    show_compile("ref_unsealed", {leaf(ORCGPU_PRED_IN_SET, "i64", 9)}, &sets);
    show_compile("ref_failed", {leaf(ORCGPU_PRED_IN_SET, "i64", 10)}, &sets);
    show_compile("ref_other_context", {leaf(ORCGPU_PRED_IN_SET, "i64", 12345)}, &sets);
    show_compile("ref_no_sets", {leaf(ORCGPU_PRED_IN_SET, "i64", 7)}, nullptr);
    show_compile("ref_children", {leaf(ORCGPU_PRED_IN_SET, "i64", 7, 1), int_lit(ORCGPU_PRED_LITERAL, nullptr, 4)}, &sets);
  }
  printf("hold_uses_after %ld\n", hold.use_count());
  char err[256];
  printf("col_dict %d\t", key_set_column_check(ORCGPU_T_INT, true, false, "d", "key set", err, sizeof(err)));
  printf("%s\n", err);
  printf("col_nested %d\t", key_set_column_check(ORCGPU_T_STRUCT, false, true, "st", "key set", err, sizeof(err)));
  printf("%s\n", err);
  printf("col_ok %d\n", key_set_column_check(ORCGPU_T_DATE, false, false, "d", "key set", err, sizeof(err)));
  return 0;
}
