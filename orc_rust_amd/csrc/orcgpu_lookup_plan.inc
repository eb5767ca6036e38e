// orcgpu_lookup_plan.inc -- key maps and lookup columns (include/orcgpu.h: "Key maps and lookup columns") as the host plans them,
// free of HIP and of the reader: which columns may be a map's value and as what they are stored (key_map_value_check), where the
// value planes lie behind a key set's table (key_map_planes), what a reader is told of a map it probes (LookupMapRef), and the
// lookup columns of a reader against its projected root columns (lookup_compile): names, probe keys, the (map, key column) pairs
// one launch serves each.  Every refusal of the lookup columns is decided here.  key_map_build_host lays a sealed map out on the
// host -- what the insert and seal kernels leave, up to where a key lies in its chain -- and key_map_probe_host answers a key with
// the probe text the kernel runs (device/key_map_program.h): tests/hostcheck/key_map_check.cpp compiles this file for the host.
#pragma once
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device/key_map_program.h"
#include "orcgpu_key_set.inc"

namespace orcgpu_host {

static_assert(ORCGPU_KEY_MAP_MAX_VALUES == kKeyMapMaxValues && ORCGPU_LOOKUP_MAX == 8, "the key map of include/orcgpu.h");
static_assert((int)ORCGPU_KEY_MAP_INT64 == (int)KMV_INT64 && (int)ORCGPU_KEY_MAP_DECIMAL128 == (int)KMV_DEC128 && (int)ORCGPU_KEY_MAP_FLOAT64 == (int)KMV_F64, "the value kinds of include/orcgpu.h");
constexpr uint32_t kLookupMaxPairs = 4;  // distinct (map, probe key column) pairs of one reader: one launch each

struct KeyMapValue {
  uint32_t kind = KMV_INT64;  // KMV_*
  uint32_t precision = 0, scale = 0;  // KMV_DEC128: the column's own
  bool operator==(const KeyMapValue& o) const { return kind == o.kind && precision == o.precision && scale == o.scale; }
};

// May a column be a value of a key map, and as what is it stored?  Byte .. Long and Date: Int64 (a Date as int64 days); Decimal(p, s):
// Decimal128(p, s); Float / Double: Float64.  ORCGPU_UNSUPPORTED with the column's name in `err` otherwise.
inline int key_map_value_check(int32_t orc_type, uint32_t precision, uint32_t scale, bool dict_read, bool nested, const char* name, KeyMapValue& out, char* err, size_t n) {
  const char* why = nullptr;
  out = KeyMapValue{};
  switch (orc_type) {
    case ORCGPU_T_BYTE: case ORCGPU_T_SHORT: case ORCGPU_T_INT: case ORCGPU_T_LONG: case ORCGPU_T_DATE: out.kind = KMV_INT64; break;
    case ORCGPU_T_DECIMAL: out.kind = KMV_DEC128, out.precision = precision, out.scale = scale; break;
    case ORCGPU_T_FLOAT: case ORCGPU_T_DOUBLE: out.kind = KMV_F64; break;
    case ORCGPU_T_TIMESTAMP: case ORCGPU_T_TIMESTAMP_INSTANT: why = "a Timestamp column"; break;
    case ORCGPU_T_BOOLEAN: why = "a Boolean column"; break;
    case ORCGPU_T_STRING: case ORCGPU_T_VARCHAR: case ORCGPU_T_CHAR: case ORCGPU_T_BINARY: why = "a String / Varchar / Char / Binary column"; break;
    default: why = "a nested column or one of an unknown kind"; break;
  }
  if (!why && nested) why = "a nested column";
  if (!why && dict_read) why = "read as a dictionary column";
  if (!why) return ORCGPU_OK;
  snprintf(err, n, "key map: value column '%s' is %s: the values of a key map are Byte, Short, Int, Long, Date, Decimal, Float and Double columns", name ? name : "", why);
  return ORCGPU_UNSUPPORTED;
}

// The value names alone: 1 .. ORCGPU_KEY_MAP_MAX_VALUES of them, none twice
inline int key_map_check_value_names(const char* const* names, uint32_t n, char* err, size_t err_len) {
  if (!names || !n) {
    snprintf(err, err_len, "key map: no value column given");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (n > ORCGPU_KEY_MAP_MAX_VALUES) {
    snprintf(err, err_len, "key map: %u value columns, at most ORCGPU_KEY_MAP_MAX_VALUES (8)", n);
    return ORCGPU_INVALID_ARGUMENT;
  }
  for (uint32_t k = 0; k < n; k++) {
    if (!names[k] || !names[k][0]) {
      snprintf(err, err_len, "key map: a value column without a name");
      return ORCGPU_INVALID_ARGUMENT;
    }
    for (uint32_t j = 0; j < k; j++)
      if (strcmp(names[j], names[k]) == 0) {
        snprintf(err, err_len, "key map: the value column '%s' is given twice", names[k]);
        return ORCGPU_INVALID_ARGUMENT;
      }
  }
  return ORCGPU_OK;
}

// The planes of a map's values, in an allocation of their own: per value n_slots + 1 entries of 8 or 16 bytes (the last: the key
// whose value is the sentinel's), then n_slots + 1 validity bytes; every part 256-byte aligned.
struct KeyMapPlanes {
  uint32_t n = 0;
  uint64_t o_values[kKeyMapMaxValues] = {}, o_valid[kKeyMapMaxValues] = {}, bytes = 0;
};
inline bool key_map_planes(uint32_t n_slots, const KeyMapValue* values, uint32_t n, KeyMapPlanes& out) {
  out = KeyMapPlanes{};
  if (!n_slots || !values || !n || n > kKeyMapMaxValues) return false;
  uint64_t off = 0;
  for (uint32_t k = 0; k < n; k++) {
    out.o_values[k] = off;
    off += ((uint64_t)n_slots + 1) * key_map_value_width(values[k].kind);
    off = (off + 255) / 256 * 256;
    out.o_valid[k] = off;
    off += (uint64_t)n_slots + 1;
    off = (off + 255) / 256 * 256;
  }
  out.n = n;
  out.bytes = off;
  return true;
}
// the bytes a map of max_keys keys takes on the device: the set's allocation and the planes'
inline uint64_t key_map_bytes(uint64_t max_keys, const KeyMapValue* values, uint32_t n) {
  KeySetLayout lay;
  KeyMapPlanes pl;
  if (!key_set_layout(max_keys, lay) || !key_map_planes(lay.n_slots, values, n, pl)) return 0;
  return lay.bytes + pl.bytes;
}

// What a reader learns of a sealed map it probes; it keeps the memory alive (hold) whatever becomes of the handle
struct LookupMapRef {
  uint64_t id = 0;
  int state = KEY_SET_BUILDING;
  bool same_ctx = true;
  bool duplicate = false;     // (a failed map: why)
  uint64_t table = 0;         // the sealed table's device address ...
  uint32_t table_bytes = 0;   // ... and its bytes
  uint32_t n_slots = 0;
  uint32_t n_values = 0;
  KeyMapValue values[kKeyMapMaxValues];
  uint64_t planes = 0;        // the planes' device address
  KeyMapPlanes lay;
  std::shared_ptr<void> hold;
};

// One lookup column as given: name, the probe key column, the map (null: none given), which of its values
struct LookupSpec {
  const char* name = nullptr;
  const char* key_column = nullptr;
  const LookupMapRef* map = nullptr;
  uint32_t value = 0;
};
// A projected root column as the lookup plan needs it
struct LookupProjCol {
  int32_t orc_type = 0;
  bool dict_read = false, nested = false;
};
struct LookupColumn {
  std::string name;
  uint32_t pair = 0, value = 0;  // which pair probes for it, which of the map's values it is
  KeyMapValue v;
};
struct LookupPair {
  uint32_t key_col = 0;  // the probe key among the projected root columns
  LookupMapRef map;
  std::vector<uint32_t> cols;  // its lookup columns (indices into LookupPlan::cols), in the order given
};
struct LookupPlan {
  std::vector<LookupColumn> cols;
  std::vector<LookupPair> pairs;
  char err[384] = "";
};

// what a lookup column is to everything that resolves names behind it: an ORC Long, Decimal(p, s) or Double
inline int32_t lookup_orc_type(const KeyMapValue& v) { return v.kind == KMV_F64 ? ORCGPU_T_DOUBLE : v.kind == KMV_DEC128 ? ORCGPU_T_DECIMAL : ORCGPU_T_LONG; }

// The names alone: 1 .. ORCGPU_LOOKUP_MAX of them, non-empty, distinct, none a root column name of the file (projected or not), none
// a computed column's name.  What the setter can refuse before the file's columns are known (file_roots: null, 0 then).
inline int lookup_check_names(const char* const* names, uint32_t n, const char* const* file_roots, uint32_t n_file_roots, const char* const* computed, uint32_t n_computed,
                              char* err, size_t err_len) {
  auto fail = [&](const char* fmt, const char* a = "") {
    snprintf(err, err_len, fmt, a);
    return (int)ORCGPU_INVALID_ARGUMENT;
  };
  if (!names || !n) return fail("lookup columns: no lookup column given");
  if (n > ORCGPU_LOOKUP_MAX) return fail("lookup columns: more than ORCGPU_LOOKUP_MAX (8) lookup columns");
  for (uint32_t k = 0; k < n; k++) {
    if (!names[k] || !names[k][0]) return fail("lookup columns: a lookup column without a name");
    for (uint32_t j = 0; j < k; j++)
      if (strcmp(names[j], names[k]) == 0) return fail("lookup columns: the name '%s' is given twice", names[k]);
    for (uint32_t j = 0; j < n_file_roots; j++)
      if (file_roots[j] && strcmp(file_roots[j], names[k]) == 0) return fail("lookup columns: '%s' is the name of a root column of the file", names[k]);
    for (uint32_t j = 0; j < n_computed; j++)
      if (computed[j] && strcmp(computed[j], names[k]) == 0) return fail("lookup columns: '%s' is the name of a computed column", names[k]);
  }
  return ORCGPU_OK;
}

// A map as a probe may use it: of this context, sealed
inline int lookup_check_map(const LookupMapRef* m, const char* name, char* err, size_t err_len) {
  const char* why = !m ? "names no key map" : !m->same_ctx ? "names a key map of another context" : m->state == KEY_SET_BUILDING ? "names a key map that is not sealed yet (orcgpu_key_map_seal)"
                    : m->state == KEY_SET_FAILED ? (m->duplicate ? "names a key map whose seal failed (duplicate key): it is unusable" : "names a key map whose seal failed (more than max_keys keys): it is unusable")
                    : nullptr;
  if (!why) return ORCGPU_OK;
  snprintf(err, err_len, "lookup column '%s' %s", name ? name : "", why);
  return ORCGPU_INVALID_ARGUMENT;
}

// specs: the n lookup columns as given.  file_roots: every root column name of the file.  computed: the reader's computed columns'
// names.  proj_names / proj_cols: the projected root columns, among which the probe keys are found.
inline int lookup_compile(const LookupSpec* specs, uint32_t n, const char* const* file_roots, uint32_t n_file_roots, const char* const* computed, uint32_t n_computed,
                          const char* const* proj_names, const LookupProjCol* proj_cols, uint32_t n_proj, LookupPlan& plan) {
  plan.cols.clear();
  plan.pairs.clear();
  plan.err[0] = 0;
  auto fail = [&](int rc, const char* fmt, const char* a = "", const char* b = "") {
    snprintf(plan.err, sizeof(plan.err), fmt, a, b);
    plan.cols.clear();  // (a refused plan holds nothing)
    plan.pairs.clear();
    return rc;
  };
  if (!specs) return fail(ORCGPU_INVALID_ARGUMENT, "lookup columns: no lookup column given");
  std::vector<const char*> names;
  for (uint32_t k = 0; k < n && k <= ORCGPU_LOOKUP_MAX; k++) names.push_back(specs[k].name);
  if (const int rc = lookup_check_names(names.data(), n, file_roots, n_file_roots, computed, n_computed, plan.err, sizeof(plan.err))) return rc;
  for (uint32_t j = 0; j < n_proj; j++)
    if (proj_cols[j].nested)
      return fail(ORCGPU_UNSUPPORTED, "lookup columns: the projected column '%s' is nested (Struct / List / Map / Union): not supported beside lookup columns", proj_names[j]);
  for (uint32_t k = 0; k < n; k++) {
    const LookupSpec& s = specs[k];
    char why[320];
    if (const int rc = lookup_check_map(s.map, s.name, why, sizeof(why))) return fail(rc, "%s", why);
    if (s.value >= s.map->n_values || s.value >= kKeyMapMaxValues) {
      char num[64];
      snprintf(num, sizeof(num), "value %u of a key map of %u values", s.value, s.map->n_values);
      return fail(ORCGPU_INVALID_ARGUMENT, "lookup column '%s' names %s", s.name, num);
    }
    if (!s.key_column || !s.key_column[0]) return fail(ORCGPU_INVALID_ARGUMENT, "lookup column '%s' names no probe key column", s.name);
    for (uint32_t j = 0; j < n; j++)
      if (strcmp(specs[j].name, s.key_column) == 0)
        return fail(ORCGPU_UNSUPPORTED, "lookup column '%s': its probe key '%s' is a lookup column: the probe key is a column of the file", s.name, s.key_column);
    for (uint32_t j = 0; j < n_computed; j++)
      if (computed[j] && strcmp(computed[j], s.key_column) == 0)
        return fail(ORCGPU_UNSUPPORTED, "lookup column '%s': its probe key '%s' is a computed column: the probe key is a column of the file", s.name, s.key_column);
    uint32_t col = n_proj;
    for (uint32_t j = 0; j < n_proj && col == n_proj; j++)
      if (proj_names[j] && strcmp(proj_names[j], s.key_column) == 0) col = j;
    if (col == n_proj) return fail(ORCGPU_INVALID_ARGUMENT, "lookup column '%s': its probe key '%s' is not a projected root column", s.name, s.key_column);
    char err[256];
    if (const int rc = key_set_column_check(proj_cols[col].orc_type, proj_cols[col].dict_read, proj_cols[col].nested, s.key_column, "lookup columns", err, sizeof(err)))
      return fail(rc, "%s", err);
    uint32_t pair = (uint32_t)plan.pairs.size();
    for (uint32_t p = 0; p < plan.pairs.size() && pair == plan.pairs.size(); p++)
      if (plan.pairs[p].key_col == col && plan.pairs[p].map.id == s.map->id) pair = p;
    if (pair == plan.pairs.size()) {
      if (pair == kLookupMaxPairs) return fail(ORCGPU_INVALID_ARGUMENT, "lookup column '%s' opens a fifth (key map, probe key) pair: at most 4 a reader", s.name);
      LookupPair p;
      p.key_col = col;
      p.map = *s.map;
      plan.pairs.push_back(std::move(p));
    }
    LookupColumn c;
    c.name = s.name;
    c.pair = pair;
    c.value = s.value;
    c.v = s.map->values[s.value];
    plan.pairs[pair].cols.push_back((uint32_t)plan.cols.size());
    plan.cols.push_back(std::move(c));
  }
  return ORCGPU_OK;
}

// A computed column's expression may not name a lookup column (in this version): the refusal, by both names
inline int lookup_refuse_computed_operand(const LookupPlan& plan, const char* computed_name, const char* operand, char* err, size_t err_len) {
  for (const LookupColumn& c : plan.cols)
    if (operand && c.name == operand) {
      snprintf(err, err_len, "computed column '%s': its operand '%s' is a lookup column: computed columns over lookup columns are not supported", computed_name ? computed_name : "", operand);
      return ORCGPU_UNSUPPORTED;
    }
  return ORCGPU_OK;
}

// ---- a sealed map on the host (for the host check): the set's table and the planes, as the kernels leave them ----
struct KeyMapHostValue {
  bool valid = false;
  uint64_t lo = 0, hi = 0;  // 8 bytes: lo
};
struct KeyMapHost {
  KeySetLayout lay;
  KeyMapPlanes pl;
  std::vector<uint64_t> table;   // (8-byte words: the probe reads them)
  std::vector<uint8_t> planes;
  std::vector<KeyMapValue> values;
};
// keys: distinct; rows[k * n_values + v]: value v of key k
inline bool key_map_build_host(const uint64_t* keys, size_t n, const KeyMapHostValue* rows, const KeyMapValue* values, uint32_t n_values, uint64_t max_keys, uint32_t hash_mask,
                               KeyMapHost& out) {
  std::vector<uint8_t> tab;
  if (!key_set_build_host(keys, n, false, max_keys, hash_mask, tab)) return false;
  key_set_layout(max_keys, out.lay);
  if (!key_map_planes(out.lay.n_slots, values, n_values, out.pl)) return false;
  out.values.assign(values, values + n_values);
  out.table.assign((tab.size() + 7) / 8, 0);
  memcpy(out.table.data(), tab.data(), tab.size());
  out.planes.assign(out.pl.bytes, 0xA5);  // (what no key owns is never read)
  const InTable t = in_table(reinterpret_cast<const uint8_t*>(out.table.data()), (uint32_t)tab.size());
  for (size_t k = 0; k < n; k++) {
    const uint32_t s = in_find_i64(t, keys[k]);
    if (s == kKeyMapNoSlot) return false;
    const uint32_t at = key_map_value_index(s, keys[k], out.lay.n_slots);
    for (uint32_t v = 0; v < n_values; v++) {
      const KeyMapHostValue& x = rows[k * n_values + v];
      const uint32_t w = key_map_value_width(values[v].kind);
      uint8_t* p = out.planes.data() + out.pl.o_values[v] + (uint64_t)at * w;
      const uint64_t lo = x.valid ? x.lo : 0, hi = x.valid ? x.hi : 0;
      memcpy(p, &lo, 8);
      if (w == 16) memcpy(p + 8, &hi, 8);
      out.planes[out.pl.o_valid[v] + at] = x.valid ? 1 : 0;
    }
  }
  return true;
}
// what lookup_columns_kernel answers for a probe key: false = NULL
inline bool key_map_probe_host(const KeyMapHost& m, uint64_t key, uint32_t v, uint64_t* lo, uint64_t* hi) {
  *lo = *hi = 0;
  InTable t = in_table(reinterpret_cast<const uint8_t*>(m.table.data()), (uint32_t)m.lay.table_bytes);
  if (t.kind != IN_KEY_I64 || t.n_slots != m.lay.n_slots || v >= m.pl.n) return false;
  const uint32_t s = in_find_i64(t, key);
  if (s == kKeyMapNoSlot) return false;
  const uint32_t at = key_map_value_index(s, key, m.lay.n_slots);
  if (!m.planes[m.pl.o_valid[v] + at]) return false;
  const uint32_t w = key_map_value_width(m.values[v].kind);
  memcpy(lo, m.planes.data() + m.pl.o_values[v] + (uint64_t)at * w, 8);
  if (w == 16) memcpy(hi, m.planes.data() + m.pl.o_values[v] + (uint64_t)at * w + 8, 8);
  return true;
}

}  // namespace orcgpu_host
