// orcgpu_group_plan.inc -- GROUP BY for the aggregates, the part that is free of HIP (tests/hostcheck/group_plan_check.cpp compiles
// this very text under AddressSanitizer + UBSan): the key list against the columns of a result -> what the kernels of
// device/agg_group_kernels.hip hash and compare, with every refusal of orcgpu_result_aggregate_groups (include/orcgpu.h) decided
// here; the merge of the stripes' groups by key tuple, in first-appearance order, with agg_merge per instruction; the cap on the
// total; the limits of a GROUP BY and, for the wide path of device/agg_group_wide_kernels.hip, its table's slots, its sort's passes
// and its workspace layout (tests/hostcheck/group_wide_check.cpp compiles those likewise); and the last step, the records -> the orcgpu_group_key and orcgpu_agg_value handed out.  Included behind
// orcgpu_agg_plan.inc, whose AggCol says what a column is.
#include <cstdlib>
#include <string>
#include <unordered_map>

#include "device/agg_group_program.h"

// What orcgpu_result_aggregate_groups and orcgpu_reader_aggregate_groups hand out: [group][key] and [group][spec]
struct orcgpu_groups {
  uint32_t n_groups = 0, n_keys = 0, n_specs = 0;
  std::vector<orcgpu_group_key> keys;
  std::vector<orcgpu_agg_value> values;
};

namespace orcgpu_host {

static_assert(sizeof(GroupKeyRecord) == 24 + ORCGPU_GROUP_KEY_BYTES && sizeof(GroupSlot) == 16 && sizeof(GroupControl) == 16,
              "agg_group_program.h: the records the kernels read and write");
static_assert(kGroupMaxKeys == ORCGPU_GROUP_MAX_KEYS && kGroupMax == ORCGPU_GROUP_MAX && kGroupKeyBytes == ORCGPU_GROUP_KEY_BYTES, "the limits of include/orcgpu.h");

struct GroupKey {
  uint32_t col = 0;            // index into the result's columns
  uint32_t fkind = 0;          // FKIND_* the kernels load it as
  uint32_t kind = 0;           // ORCGPU_GROUP_KEY_*
  int32_t scale_or_unit = -1;  // Decimal: the scale; Timestamp: the unit
};
struct GroupPlan {
  std::vector<GroupKey> keys;
  uint32_t max_groups = ORCGPU_GROUP_MAX;       // the limits: groups of one result (above kGroupMax: the wide path) ...
  uint32_t max_total = ORCGPU_GROUP_MAX_TOTAL;  // ... and over a reader's stripes (group_limits)
  char err[256] = {0};
};

// ---- the limits, and what the wide path (device/agg_group_wide_kernels.hip) is sized by: plain arithmetic ----
static_assert(kGroupLimitMax == ORCGPU_GROUP_LIMIT_MAX && kGroupLimitMax <= ORCGPU_GROUP_TOTAL_LIMIT_MAX, "the limits of include/orcgpu.h");

// The limits as given (0: the default) -> max_groups / max_total; ORCGPU_INVALID_ARGUMENT with a message for a value above its
// maximum, and for a total below the limit of one result
inline int group_limits(uint32_t max_groups, uint32_t max_total, uint32_t* out_groups, uint32_t* out_total, char* err, size_t err_len) {
  const uint32_t g = max_groups ? max_groups : ORCGPU_GROUP_MAX, t = max_total ? max_total : ORCGPU_GROUP_MAX_TOTAL;
  if (g > ORCGPU_GROUP_LIMIT_MAX) {
    snprintf(err, err_len, "group by: a limit of %u groups in one result is above ORCGPU_GROUP_LIMIT_MAX (%u)", g, (unsigned)ORCGPU_GROUP_LIMIT_MAX);
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (t > ORCGPU_GROUP_TOTAL_LIMIT_MAX) {
    snprintf(err, err_len, "group by: a limit of %u groups over the stripes is above ORCGPU_GROUP_TOTAL_LIMIT_MAX (%u)", t, (unsigned)ORCGPU_GROUP_TOTAL_LIMIT_MAX);
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (t < g) {
    snprintf(err, err_len, "group by: a limit of %u groups over the stripes is below the limit of %u groups in one result", t, g);
    return ORCGPU_INVALID_ARGUMENT;
  }
  *out_groups = g;
  *out_total = t;
  return ORCGPU_OK;
}
// Which path a call takes: the limit alone decides, never the data
inline bool group_is_wide(uint32_t max_groups) { return max_groups > kGroupMax; }
// The slots of the wide path's table: the power of two >= 4 x the limit (the narrow path's 1024 at 256)
inline uint32_t group_wide_slots(uint32_t max_groups) {
  uint32_t s = 4;
  while (s < 4ull * max_groups) s <<= 1;
  return s;
}
// The passes of its sort: kGroupRadixBits bits of the group number each, as many as the numbers below the limit hold
inline uint32_t group_wide_passes(uint32_t max_groups) {
  uint32_t bits = 0;
  while ((1ull << bits) < max_groups) bits++;
  const uint32_t p = (bits + kGroupRadixBits - 1) / kGroupRadixBits;
  return p ? p : 1;
}
// Where its tables lie behind `base` (every offset aligned to kFilterAlign, in this order, none overlapping; bytes: the end).
// tiles: the blocks of the kernels that take a tile each; cap: the groups the records have room for -- a result holds no more
// groups than the limit allows, nor than it has input rows.  [o_ctl, + sizeof(GroupControl)) is what the first wait fetches;
// the second fetches n_groups records from o_key_recs ([group][key]) and from o_vals ([group][instruction]).
struct GroupWideLayout {
  uint32_t slots = 0, passes = 0, tiles = 0, cap = 0;
  uint64_t o_table = 0, table_bytes = 0, o_plane = 0, o_slot_group = 0, o_blk_first = 0, o_blk_kept = 0, o_keys[2] = {0, 0}, o_rows[2] = {0, 0}, o_hist = 0, o_seg = 0,
           o_ctl = 0, o_key_recs = 0, o_vals = 0, bytes = 0;
};
inline GroupWideLayout group_wide_layout(uint64_t base, uint32_t max_groups, uint64_t n_in, uint32_t n_insn, uint32_t n_keys) {
  GroupWideLayout w;
  FilterBump t;
  t.off = base;
  const uint64_t padded = (n_in + 63) / 64 * 64, tiles = (n_in + kGroupWideTile - 1) / kGroupWideTile;
  w.slots = group_wide_slots(max_groups);
  w.passes = group_wide_passes(max_groups);
  w.tiles = (uint32_t)(tiles ? tiles : 1);
  w.cap = (uint32_t)(n_in < max_groups ? n_in : max_groups);
  w.table_bytes = (uint64_t)w.slots * sizeof(GroupSlot);
  w.o_table = t.take(w.table_bytes);
  w.o_plane = t.take(padded * 4);
  w.o_slot_group = t.take((uint64_t)w.slots * 4);
  w.o_blk_first = t.take((uint64_t)w.tiles * 4);
  w.o_blk_kept = t.take((uint64_t)w.tiles * 4);
  for (int k = 0; k < 2; k++) w.o_keys[k] = t.take(padded * 4);
  for (int k = 0; k < 2; k++) w.o_rows[k] = t.take(padded * 4);
  w.o_hist = t.take((uint64_t)w.tiles * 256 * 4);
  w.o_seg = t.take((uint64_t)w.cap * 4);
  w.o_ctl = t.take(sizeof(GroupControl));
  w.o_key_recs = t.take((uint64_t)w.cap * n_keys * sizeof(GroupKeyRecord));
  w.o_vals = t.take((uint64_t)w.cap * n_insn * sizeof(AggPartial));
  w.bytes = t.take(0);
  return w;
}

// The key compiler: names / cols are the result's columns, as for agg_compile
inline int group_compile(const char* const* key_columns, uint32_t n_keys, const char* const* names, const AggCol* cols, uint32_t n_columns, GroupPlan& out) {
  out.keys.clear();
  out.err[0] = 0;
  auto fail = [&](int rc, const char* fmt, const char* a = "") {
    snprintf(out.err, sizeof(out.err), fmt, a);
    return rc;
  };
  if (!key_columns || !n_keys) return fail(ORCGPU_INVALID_ARGUMENT, "group by: no key column given%s");
  if (n_keys > ORCGPU_GROUP_MAX_KEYS) return fail(ORCGPU_INVALID_ARGUMENT, "group by: more than ORCGPU_GROUP_MAX_KEYS (4) key columns%s");
  for (uint32_t k = 0; k < n_columns; k++)
    if (cols[k].nested)
      return fail(ORCGPU_UNSUPPORTED, "group by: the result holds the nested column '%s' (Struct / List / Map / Union are not aggregated)", names[k] ? names[k] : "");
  for (uint32_t q = 0; q < n_keys; q++) {
    const char* name = key_columns[q];
    if (!name) return fail(ORCGPU_INVALID_ARGUMENT, "group by: a key without a column name%s");
    GroupKey key;
    uint32_t col = n_columns;
    for (uint32_t k = 0; k < n_columns && col == n_columns; k++)
      if (names[k] && strcmp(names[k], name) == 0) col = k;
    if (col == n_columns) return fail(ORCGPU_INVALID_ARGUMENT, "group by: key column '%s' is not a projected root column", name);
    for (const GroupKey& seen : out.keys)
      if (seen.col == col) return fail(ORCGPU_INVALID_ARGUMENT, "group by: key column '%s' is listed twice", name);
    const AggCol& c = cols[col];
    key.col = col;
    if (c.d.dict_out) return fail(ORCGPU_UNSUPPORTED, "group by: key column '%s' is read as a dictionary column: grouping by its keys is not supported", name);
    const int32_t t = c.d.orc_type;
    const int cls = agg_class(t);
    if (cls == ACLASS_FLOAT) return fail(ORCGPU_MISMATCHED_SCHEMA, "group by: key column '%s' is a Float / Double column", name);
    if (t == ORCGPU_T_BINARY) return fail(ORCGPU_MISMATCHED_SCHEMA, "group by: key column '%s' is a Binary column", name);
    if (cls == ACLASS_TS && (c.d.ts_unit > 3 || c.d.width != 8))
      return fail(ORCGPU_UNSUPPORTED, "group by: key column '%s' is a Timestamp decoded to Decimal128(38, 9): it is not supported as a key", name);
    uint32_t want = FKIND_INT;
    if (t == ORCGPU_T_STRING || t == ORCGPU_T_VARCHAR || t == ORCGPU_T_CHAR) {
      key.kind = ORCGPU_GROUP_KEY_STRING;
      want = FKIND_STRING;
    } else if (cls == ACLASS_BOOL) {
      key.kind = ORCGPU_GROUP_KEY_BOOL;
      want = FKIND_BOOL;
    } else if (cls == ACLASS_DEC) {
      key.kind = ORCGPU_GROUP_KEY_DEC128;
      key.scale_or_unit = (int32_t)c.scale;
      want = FKIND_DEC128;
    } else if (cls == ACLASS_INT || cls == ACLASS_DATE || cls == ACLASS_TS) {
      key.kind = ORCGPU_GROUP_KEY_I64;
      if (cls == ACLASS_TS) key.scale_or_unit = c.d.ts_unit;
    } else {
      return fail(ORCGPU_MISMATCHED_SCHEMA, "group by: key column '%s' is of a kind that cannot be a key", name);
    }
    // ... and what the decode made of it must be what the kernels load
    if (filter_col_kind(c.d) != want) return fail(ORCGPU_MISMATCHED_SCHEMA, "group by: key column '%s' is not decoded to the type a key of its kind needs", name);
    key.fkind = want;
    out.keys.push_back(key);
  }
  return ORCGPU_OK;
}

// The groups of one result or of the stripes merged so far, in first-appearance order: keys [group][key], values [group][instruction]
struct GroupSet {
  uint32_t n_keys = 0, n_insn = 0;
  std::vector<GroupKeyRecord> keys;
  std::vector<AggPartial> vals;
  std::unordered_map<std::string, uint32_t> index;  // (the merge's: key tuple -> group)
  uint32_t n_groups() const { return n_keys ? (uint32_t)(keys.size() / n_keys) : 0; }
};

// A key tuple as bytes: per key the validity, then the 16-byte value or the length and the bytes -- so that NULL, 0 and the empty
// string are three different keys, and so are ("a", "bc") and ("ab", "c")
inline std::string group_tuple(const GroupPlan& plan, const GroupKeyRecord* rec) {
  std::string s;
  for (size_t k = 0; k < plan.keys.size(); k++) {
    const GroupKeyRecord& r = rec[k];
    s.push_back(r.is_null ? 0 : 1);
    if (r.is_null) continue;
    if (plan.keys[k].kind == ORCGPU_GROUP_KEY_STRING) {
      const uint32_t len = r.len < kGroupKeyBytes ? r.len : kGroupKeyBytes;
      s.append(reinterpret_cast<const char*>(&len), 4);
      s.append(reinterpret_cast<const char*>(r.bytes), len);
    } else {
      s.append(reinterpret_cast<const char*>(r.w), 16);
    }
  }
  return s;
}

// total <- total merged with the groups of a later stripe (its keys [group][key], vals [group][instruction], n groups): a key seen
// before folds into its group with agg_merge, a new one goes behind the groups so far.  ORCGPU_UNSUPPORTED when the total
// passes the plan's max_total (ORCGPU_GROUP_MAX_TOTAL unless it was set); `total` is then no longer of use.  Linear in the
// groups offered: the index grows by doubling, so that a stripe of a million groups rehashes it once at the most.
inline int group_merge(const GroupPlan& plan, const std::vector<AggInsn>& insns, GroupSet& total, const GroupKeyRecord* keys, const AggPartial* vals, uint32_t n,
                       char* err, size_t err_len) {
  const uint32_t nk = (uint32_t)plan.keys.size(), ni = (uint32_t)insns.size();
  total.n_keys = nk;
  total.n_insn = ni;
  {
    const size_t have = total.index.size(), want = have + n < plan.max_total ? have + n : (size_t)plan.max_total + 1;
    if ((double)want > (double)total.index.bucket_count() * total.index.max_load_factor()) total.index.reserve(want > 2 * have ? want : 2 * have);
  }
  for (uint32_t g = 0; g < n; g++) {
    const std::string tuple = group_tuple(plan, keys + (size_t)g * nk);
    auto it = total.index.find(tuple);
    if (it == total.index.end()) {
      const uint32_t at = total.n_groups();
      if (at >= plan.max_total) {
        snprintf(err, err_len, "group by: more than %u groups over the stripes (the limit set; ORCGPU_GROUP_MAX_TOTAL by default)", plan.max_total);
        return ORCGPU_UNSUPPORTED;
      }
      total.index.emplace(tuple, at);
      total.keys.insert(total.keys.end(), keys + (size_t)g * nk, keys + (size_t)(g + 1) * nk);
      total.vals.insert(total.vals.end(), vals + (size_t)g * ni, vals + (size_t)(g + 1) * ni);
      continue;
    }
    for (uint32_t k = 0; k < ni; k++) agg_merge(insns[k], total.vals[(size_t)it->second * ni + k], vals[(size_t)g * ni + k]);
  }
  return ORCGPU_OK;
}

// A key record -> what the caller gets
inline void group_key_finish(const GroupKey& key, const GroupKeyRecord& r, orcgpu_group_key* out) {
  memset(out, 0, sizeof(*out));
  out->kind = key.kind;
  out->scale_or_unit = key.scale_or_unit;
  out->is_null = r.is_null ? 1 : 0;
  if (r.is_null) return;
  if (key.kind == ORCGPU_GROUP_KEY_STRING) {
    out->len = r.len < kGroupKeyBytes ? r.len : kGroupKeyBytes;
    memcpy(out->bytes, r.bytes, out->len);
  } else {
    out->w[0] = r.w[0];
    out->w[1] = r.w[1];
  }
}

// The finish step: the first n_specs instructions of every group through agg_finish (what stands behind them -- the kept row
// count -- is the caller's), the keys through group_key_finish
inline void group_finish(const GroupPlan& plan, const std::vector<AggInsn>& insns, uint32_t n_specs, const GroupSet& set, orcgpu_groups& out) {
  const uint32_t nk = (uint32_t)plan.keys.size(), ni = (uint32_t)insns.size(), n = set.n_groups();
  out.n_groups = n;
  out.n_keys = nk;
  out.n_specs = n_specs;
  out.keys.assign((size_t)n * nk, orcgpu_group_key{});
  out.values.assign((size_t)n * n_specs, orcgpu_agg_value{});
  for (uint32_t g = 0; g < n; g++) {
    for (uint32_t k = 0; k < nk; k++) group_key_finish(plan.keys[k], set.keys[(size_t)g * nk + k], &out.keys[(size_t)g * nk + k]);
    for (uint32_t k = 0; k < n_specs && k < ni; k++) agg_finish(insns[k], set.vals[(size_t)g * ni + k], &out.values[(size_t)g * n_specs + k]);
  }
}

// What the device's flags say of a result, or ORCGPU_OK: names are the result's columns
inline int group_check_flags(const GroupPlan& plan, uint32_t flags, uint32_t n_groups, const char* const* names, char* err, size_t err_len) {
  if ((flags & GROUP_TOO_MANY) || n_groups > plan.max_groups) {
    snprintf(err, err_len, "group by: more than %u groups in one stripe (the limit set; ORCGPU_GROUP_MAX by default)", plan.max_groups);
    return ORCGPU_UNSUPPORTED;
  }
  for (size_t k = 0; k < plan.keys.size(); k++)
    if (flags & ((uint32_t)GROUP_KEY_TOO_LONG << k)) {
      snprintf(err, err_len, "group by: key column '%s' holds a value of more than ORCGPU_GROUP_KEY_BYTES (%u) bytes among the kept rows", names[plan.keys[k].col], kGroupKeyBytes);
      return ORCGPU_UNSUPPORTED;
    }
  return ORCGPU_OK;
}

// ORCGPU_GROUP_HASH_BITS=N -> the mask of the hash bits kept (anything else: all 32)
inline uint32_t group_hash_mask(const char* env) {
  if (!env || !*env) return 0xffffffffu;
  const long n = strtol(env, nullptr, 10);
  return n >= 1 && n < 32 ? (uint32_t)((1ull << n) - 1) : 0xffffffffu;
}

}  // namespace orcgpu_host
