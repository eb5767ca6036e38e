// key_map_check.cpp -- the host side of the key maps and lookup columns (orc_rust_amd/csrc/orcgpu_lookup_plan.inc and the probe of
// device/key_map_program.h, the very text liborcgpu.so is built from) under AddressSanitizer + UBSan, on the CPU (TEST
// INFRASTRUCTURE).  A stand-alone program: it builds its cases itself and prints one line per fact,
// "<name> <values ...>[\t<message>]"; tests/test_key_map_host_sanitized.py holds the lines to what include/orcgpu.h says and to
// tests/key_map_model.py.  "probe" cases come on the command line:
//   probe <name> <max_keys> <hash bits, 0: all> <n keys> {<key> <v0: int64 | n> <v1: hex bits of a double | n>}... <probe key>...
// and print, per probe key, "<v0 | n>:<v1 | n>".  Exit code 0 when it ran through; a sanitizer report aborts with its own code.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/orcgpu.h"
#include "../../orc_rust_amd/csrc/orcgpu_lookup_plan.inc"

using namespace orcgpu_host;

static KeyMapValue val(uint32_t kind, uint32_t p = 0, uint32_t s = 0) {
  KeyMapValue v;
  v.kind = kind, v.precision = p, v.scale = s;
  return v;
}

static void show_planes(const char* name, uint64_t max_keys, const std::vector<KeyMapValue>& values) {
  KeySetLayout lay;
  KeyMapPlanes pl;
  const bool ok = key_set_layout(max_keys, lay) && key_map_planes(lay.n_slots, values.data(), (uint32_t)values.size(), pl);
  printf("%s %d %u %llu %llu", name, ok ? 1 : 0, lay.n_slots, (unsigned long long)pl.bytes, (unsigned long long)key_map_bytes(max_keys, values.data(), (uint32_t)values.size()));
  for (uint32_t k = 0; ok && k < pl.n; k++) printf(" %llu:%llu", (unsigned long long)pl.o_values[k], (unsigned long long)pl.o_valid[k]);
  printf("\n");
}

// the projected root columns of the plan cases
static const char* const kProj[] = {"i8", "i16", "i32", "i64", "date", "ts", "dec", "f64", "b", "s", "dict"};
static const char* const kRoots[] = {"i8", "i16", "i32", "i64", "date", "ts", "dec", "f64", "b", "s", "dict", "unprojected"};
static std::vector<LookupProjCol> proj_cols(bool with_struct) {
  const int32_t kinds[] = {ORCGPU_T_BYTE, ORCGPU_T_SHORT, ORCGPU_T_INT, ORCGPU_T_LONG, ORCGPU_T_DATE, ORCGPU_T_TIMESTAMP, ORCGPU_T_DECIMAL, ORCGPU_T_DOUBLE,
                           ORCGPU_T_BOOLEAN, ORCGPU_T_STRING, ORCGPU_T_INT};
  std::vector<LookupProjCol> out(11);
  for (int k = 0; k < 11; k++) out[k].orc_type = kinds[k];
  out[10].dict_read = true;
  if (with_struct) out[9].orc_type = ORCGPU_T_STRUCT, out[9].nested = true;
  return out;
}
static LookupMapRef sealed_map(uint64_t id, std::shared_ptr<void> hold) {
  LookupMapRef m;
  m.id = id, m.state = KEY_SET_SEALED, m.table = 0x7f0000001000ull + id * 0x10000, m.table_bytes = 32 + 8 + 64 * 8, m.n_slots = 64, m.n_values = 3;
  m.values[0] = val(KMV_INT64), m.values[1] = val(KMV_DEC128, 12, 2), m.values[2] = val(KMV_F64);
  key_map_planes(64, m.values, 3, m.lay);
  m.planes = 0x7f0001000000ull;
  m.hold = hold;
  return m;
}
struct Spec {
  const char* name;
  const char* key;
  const LookupMapRef* map;
  uint32_t value;
};
// rc, n columns, n pairs, per column name:pair:value:kind:precision:scale, per pair key_col:map id:n cols
static void show_plan(const char* name, const std::vector<Spec>& specs, const std::vector<const char*>& computed = {}, bool with_struct = false) {
  std::vector<LookupSpec> in(specs.size());
  for (size_t k = 0; k < specs.size(); k++) in[k].name = specs[k].name, in[k].key_column = specs[k].key, in[k].map = specs[k].map, in[k].value = specs[k].value;
  const std::vector<LookupProjCol> pc = proj_cols(with_struct);
  LookupPlan plan;
  const int rc = lookup_compile(in.data(), (uint32_t)in.size(), kRoots, 12, computed.data(), (uint32_t)computed.size(), kProj, pc.data(), 11, plan);
  printf("%s %d %zu %zu", name, rc, plan.cols.size(), plan.pairs.size());
  if (!rc) {
    for (const LookupColumn& c : plan.cols) printf(" %s:%u:%u:%u:%u:%u", c.name.c_str(), c.pair, c.value, c.v.kind, c.v.precision, c.v.scale);
    for (const LookupPair& p : plan.pairs) printf(" %u:%llu:%zu", p.key_col, (unsigned long long)p.map.id, p.cols.size());
  }
  printf("\t%s\n", plan.err);
}

static void show_value(const char* name, int32_t orc_type, bool dict, bool nested) {
  KeyMapValue v;
  char err[320] = "";
  const int rc = key_map_value_check(orc_type, 12, 2, dict, nested, "c", v, err, sizeof(err));
  printf("%s %d %u %u %u\t%s\n", name, rc, v.kind, v.precision, v.scale, err);
}

// argv: see the head comment
static int run_probe(int argc, char** argv, int at) {
  const char* name = argv[at++];
  const uint64_t max_keys = strtoull(argv[at++], nullptr, 10);
  const long bits = strtol(argv[at++], nullptr, 10);
  const size_t n = strtoull(argv[at++], nullptr, 10);
  const uint32_t hash_mask = bits >= 1 && bits < 32 ? (uint32_t)((1ull << bits) - 1) : 0xffffffffu;
  std::vector<uint64_t> keys;
  std::vector<KeyMapHostValue> rows;
  for (size_t k = 0; k < n && at + 2 < argc; k++) {
    keys.push_back((uint64_t)strtoll(argv[at++], nullptr, 10));
    KeyMapHostValue a, b;
    if (strcmp(argv[at], "n")) a.valid = true, a.lo = (uint64_t)strtoll(argv[at], nullptr, 10);
    at++;
    if (strcmp(argv[at], "n")) b.valid = true, b.lo = strtoull(argv[at], nullptr, 16);
    at++;
    rows.push_back(a), rows.push_back(b);
  }
  const KeyMapValue values[2] = {val(KMV_INT64), val(KMV_F64)};
  KeyMapHost m;
  const bool built = key_map_build_host(keys.data(), keys.size(), rows.data(), values, 2, max_keys, hash_mask, m);
  printf("probe %s %d", name, built ? 1 : 0);
  for (; built && at < argc && strcmp(argv[at], "probe"); at++) {
    const uint64_t key = (uint64_t)strtoll(argv[at], nullptr, 10);
    uint64_t lo, hi;
    if (key_map_probe_host(m, key, 0, &lo, &hi)) printf(" %lld:", (long long)lo);
    else printf(" n:");
    if (key_map_probe_host(m, key, 1, &lo, &hi)) printf("%llx", (unsigned long long)lo);
    else printf("n");
  }
  printf("\n");
  while (at < argc && strcmp(argv[at], "probe")) at++;
  return at;
}

int main(int argc, char** argv) {
  // ---- plane offsets and bytes per max_keys and value list ----
  show_planes("planes_1_i64", 1, {val(KMV_INT64)});
  show_planes("planes_32_mixed", 32, {val(KMV_INT64), val(KMV_DEC128, 12, 2), val(KMV_F64)});
  show_planes("planes_33_dec", 33, {val(KMV_DEC128, 38, 0)});
  show_planes("planes_1M_eight", 1u << 20, std::vector<KeyMapValue>(8, val(KMV_DEC128, 38, 0)));
  show_planes("planes_none", 32, {});
  show_planes("planes_nine", 32, std::vector<KeyMapValue>(9, val(KMV_INT64)));
  show_planes("planes_0_keys", 0, {val(KMV_INT64)});

  // ---- which columns may be a value ----
  show_value("val_byte", ORCGPU_T_BYTE, false, false);
  show_value("val_date", ORCGPU_T_DATE, false, false);
  show_value("val_dec", ORCGPU_T_DECIMAL, false, false);
  show_value("val_float", ORCGPU_T_FLOAT, false, false);
  show_value("val_bool", ORCGPU_T_BOOLEAN, false, false);
  show_value("val_string", ORCGPU_T_STRING, false, false);
  show_value("val_ts", ORCGPU_T_TIMESTAMP, false, false);
  show_value("val_dict", ORCGPU_T_STRING, true, false);
  show_value("val_dict_int", ORCGPU_T_INT, true, false);
  show_value("val_nested", ORCGPU_T_STRUCT, false, true);
  {
    char err[256] = "";
    const char* const twice[] = {"a", "b", "a"};
    const char* const nine[] = {"a", "b", "c", "d", "e", "f", "g", "h", "i"};
    printf("names_twice %d\t", key_map_check_value_names(twice, 3, err, sizeof(err)));
    printf("%s\n", err);
    printf("names_nine %d\t", key_map_check_value_names(nine, 9, err, sizeof(err)));
    printf("%s\n", err);
    printf("names_none %d\t", key_map_check_value_names(nine, 0, err, sizeof(err)));
    printf("%s\n", err);
    printf("names_eight %d\n", key_map_check_value_names(nine, 8, err, sizeof(err)));
  }

  // ---- the lookup plan against a root table ----
  auto hold = std::make_shared<int>(0);
  {
    const LookupMapRef m1 = sealed_map(7, hold), m2 = sealed_map(8, hold);
    LookupMapRef open = sealed_map(9, hold), failed = sealed_map(10, hold), dup = sealed_map(11, hold), foreign = sealed_map(12, hold);
    open.state = KEY_SET_BUILDING, failed.state = KEY_SET_FAILED, dup.state = KEY_SET_FAILED, dup.duplicate = true, foreign.same_ctx = false;
    show_plan("plan_one", {{"x", "i64", &m1, 0}});
    show_plan("plan_pair_shares_probe", {{"x", "i64", &m1, 0}, {"y", "i64", &m1, 1}, {"z", "i64", &m1, 2}});
    show_plan("plan_two_maps", {{"x", "i64", &m1, 0}, {"y", "i32", &m2, 2}, {"z", "i64", &m1, 1}});
    show_plan("plan_same_map_two_keys", {{"x", "i8", &m1, 0}, {"y", "date", &m1, 0}});
    show_plan("plan_with_computed", {{"x", "i16", &m1, 0}}, {"c1", "c2"});
    show_plan("plan_eight", {{"la", "i8", &m1, 0}, {"lb", "i8", &m1, 1}, {"lc", "i16", &m1, 0}, {"ld", "i16", &m1, 1}, {"le", "i32", &m2, 0},
                             {"lf", "i32", &m2, 1}, {"lg", "i64", &m2, 0}, {"lh", "i64", &m2, 2}});
    printf("hold_uses %ld\n", hold.use_count());
    // every refusal with a fragment of its message
    show_plan("ref_none", {});
    show_plan("ref_nine", {{"la", "i8", &m1, 0}, {"lb", "i8", &m1, 0}, {"lc", "i8", &m1, 0}, {"ld", "i8", &m1, 0}, {"le", "i8", &m1, 0}, {"lf", "i8", &m1, 0},
                           {"lg", "i8", &m1, 0}, {"lh", "i8", &m1, 0}, {"li", "i8", &m1, 0}});
    show_plan("ref_empty_name", {{"", "i64", &m1, 0}});
    show_plan("ref_twice", {{"x", "i64", &m1, 0}, {"x", "i64", &m1, 1}});
    show_plan("ref_root_name", {{"i32", "i64", &m1, 0}});
    show_plan("ref_root_name_unprojected", {{"unprojected", "i64", &m1, 0}});
    show_plan("ref_computed_name", {{"c1", "i64", &m1, 0}}, {"c1"});
    show_plan("ref_no_map", {{"x", "i64", nullptr, 0}});
    show_plan("ref_unsealed", {{"x", "i64", &open, 0}});
    show_plan("ref_failed", {{"x", "i64", &failed, 0}});
    show_plan("ref_duplicate", {{"x", "i64", &dup, 0}});
    show_plan("ref_other_context", {{"x", "i64", &foreign, 0}});
    show_plan("ref_value_index", {{"x", "i64", &m1, 3}});
    show_plan("ref_no_key", {{"x", "", &m1, 0}});
    show_plan("ref_unknown_key", {{"x", "nope", &m1, 0}});
    show_plan("ref_unprojected_key", {{"x", "unprojected", &m1, 0}});
    show_plan("ref_lookup_key", {{"x", "i64", &m1, 0}, {"y", "x", &m1, 1}});
    show_plan("ref_computed_key", {{"x", "c1", &m1, 0}}, {"c1"});
    show_plan("ref_ts_key", {{"x", "ts", &m1, 0}});
    show_plan("ref_dec_key", {{"x", "dec", &m1, 0}});
    show_plan("ref_f64_key", {{"x", "f64", &m1, 0}});
    show_plan("ref_bool_key", {{"x", "b", &m1, 0}});
    show_plan("ref_string_key", {{"x", "s", &m1, 0}});
    show_plan("ref_dict_key", {{"x", "dict", &m1, 0}});
    show_plan("ref_nested_projection", {{"x", "i64", &m1, 0}}, {}, true);
    show_plan("ref_fifth_pair", {{"la", "i8", &m1, 0}, {"lb", "i16", &m1, 0}, {"lc", "i32", &m1, 0}, {"ld", "i64", &m1, 0}, {"le", "date", &m1, 0}});
    LookupPlan plan;
    const LookupSpec one = {"x", "i64", &m1, 0};
    const std::vector<LookupProjCol> pc = proj_cols(false);
    lookup_compile(&one, 1, kRoots, 12, nullptr, 0, kProj, pc.data(), 11, plan);
    char err[320] = "";
    printf("computed_over_lookup %d\t", lookup_refuse_computed_operand(plan, "r", "x", err, sizeof(err)));
    printf("%s\n", err);
    printf("computed_over_file %d\n", lookup_refuse_computed_operand(plan, "r", "i64", err, sizeof(err)));
  }
  printf("hold_uses_after %ld\n", hold.use_count());

  // ---- tables laid out on the host, probed by the probe text the kernel runs ----
  for (int at = 1; at < argc;) {
    if (strcmp(argv[at], "probe") || at + 4 >= argc) return 2;
    at = run_probe(argc, argv, at + 1);
  }
  return 0;
}
