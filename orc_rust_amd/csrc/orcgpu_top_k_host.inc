// orcgpu_top_k_host.inc -- what ORDER BY ... LIMIT k works out on the host, free of HIP (tests/hostcheck/top_k_host_check.cpp compiles
// this very text under AddressSanitizer + UBSan): a list of orcgpu_sort_key against the columns of a result -> the keys the kernels
// take (device/top_k_program.h), with every refusal of include/orcgpu.h's "Top-k" decided here; the pass plan -- which byte of which
// key every launch of the select and of the sort reads --; where the selection's tables lie behind the filter's workspace
// (TopKWorkspace); and the KEY RECORD with its comparison and the k-way merge of the stripes' records (top_k_merge), which is all
// orcgpu_reader_top_k_order does.  Included behind orcgpu_agg_plan.inc, whose AggCol says what a column of the result is.
//
// The key record of a handed-out row is its key string (top_k_program.h), top_k_stride(len) bytes apart: two rows compare as their
// records' first `len` bytes do, as unsigned bytes -- memcmp --, and rows with equal records are equal in every key.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <queue>
#include <vector>

#include "device/top_k_program.h"

namespace orcgpu_host {

static_assert(kTopKMaxKeys == ORCGPU_TOP_K_MAX_KEYS && kTopKMax == ORCGPU_TOP_K_MAX, "top_k_program.h states the limits of include/orcgpu.h");
static_assert(sizeof(TopKKey) == 24 && sizeof(TopKKeys) == 8 + 4 * 24, "top_k_program.h: the kernel arguments");

struct TopKPlan {
  TopKKeys keys{};
  uint32_t k = 0;
  char err[256] = {0};
};

inline int top_k_fail(TopKPlan& out, int rc, const char* fmt, const char* a = "") {
  snprintf(out.err, sizeof(out.err), fmt, a);
  return rc;
}

// keys[0 .. n_keys) against the result's columns (names[c], cols[c]) -> out.  The refusals, each beginning "top-k:".
inline int top_k_compile(const orcgpu_sort_key* keys, uint32_t n_keys, uint32_t k, const char* const* names, const AggCol* cols, uint32_t n_columns, TopKPlan& out) {
  out = TopKPlan{};
  if (!keys || !n_keys) return top_k_fail(out, ORCGPU_INVALID_ARGUMENT, "top-k: no sort key given");
  if (n_keys > kTopKMaxKeys) return top_k_fail(out, ORCGPU_INVALID_ARGUMENT, "top-k: more than ORCGPU_TOP_K_MAX_KEYS (4) sort keys");
  if (!k || k > kTopKMax) return top_k_fail(out, ORCGPU_INVALID_ARGUMENT, "top-k: k must be 1 .. ORCGPU_TOP_K_MAX (65536)");
  for (uint32_t c = 0; c < n_columns; c++)
    if (cols[c].nested)
      return top_k_fail(out, ORCGPU_UNSUPPORTED, "top-k: the result holds the nested column '%s' (Struct / List / Map / Union are not selected from)", names[c] ? names[c] : "");
  out.k = k;
  out.keys.n = n_keys;
  uint32_t at = 0;
  for (uint32_t q = 0; q < n_keys; q++) {
    const char* name = keys[q].column;
    if (!name) return top_k_fail(out, ORCGPU_INVALID_ARGUMENT, "top-k: a sort key without a column name");
    uint32_t col = n_columns;
    for (uint32_t c = 0; c < n_columns && col == n_columns; c++)
      if (names[c] && strcmp(names[c], name) == 0) col = c;
    if (col == n_columns) return top_k_fail(out, ORCGPU_INVALID_ARGUMENT, "top-k: column '%s' is not a projected root column", name);
    for (uint32_t x = 0; x < q; x++)
      if (out.keys.key[x].col == col) return top_k_fail(out, ORCGPU_INVALID_ARGUMENT, "top-k: column '%s' is listed twice", name);
    const FilterColDesc& d = cols[col].d;
    if (d.dict_out) return top_k_fail(out, ORCGPU_UNSUPPORTED, "top-k: column '%s' is read as a dictionary column: a sort key on its keys is not supported", name);
    const int t = d.orc_type;
    if (d.is_string || t == ORCGPU_T_STRING || t == ORCGPU_T_VARCHAR || t == ORCGPU_T_CHAR || t == ORCGPU_T_BINARY)
      return top_k_fail(out, ORCGPU_UNSUPPORTED, "top-k: column '%s' is a String / Varchar / Char / Binary column: string sort keys are not supported", name);
    if ((t == ORCGPU_T_TIMESTAMP || t == ORCGPU_T_TIMESTAMP_INSTANT) && (d.ts_unit > 3 || d.width != 8))
      return top_k_fail(out, ORCGPU_UNSUPPORTED, "top-k: column '%s' is a Timestamp decoded to Decimal128(38, 9): a sort key on it is not supported", name);
    const uint32_t fk = filter_col_kind(d);
    if (fk != FKIND_INT && fk != FKIND_BOOL && fk != FKIND_FLOAT && fk != FKIND_DEC128)
      return top_k_fail(out, ORCGPU_MISMATCHED_SCHEMA, "top-k: column '%s' is not decoded to a type a sort key takes", name);
    TopKKey& key = out.keys.key[q];
    key.col = col;
    key.kind = fk == FKIND_INT ? TK_INT : fk == FKIND_BOOL ? TK_BOOL : fk == FKIND_FLOAT ? TK_FLOAT : TK_DEC128;
    key.descending = keys[q].descending ? 1 : 0;
    key.nulls_first = keys[q].nulls_first ? 1 : 0;
    key.first = at;
    key.bytes = key.kind == TK_DEC128 ? 17 : 9;
    at += key.bytes;
  }
  out.keys.len = at;
  return ORCGPU_OK;
}
// The FKIND_* a key's column must have been decoded to (what the call checks in front of every launch)
inline uint32_t top_k_fkind(const TopKKey& k) { return k.kind == TK_INT ? FKIND_INT : k.kind == TK_BOOL ? FKIND_BOOL : k.kind == TK_FLOAT ? FKIND_FLOAT : FKIND_DEC128; }

// ---- the pass plan: what the launches read, from the key kinds alone ----
struct TopKPass {
  uint32_t key, byte;  // byte `byte` (0: the null byte) of key `key`: byte keys.key[key].first + byte of the key string
};
inline TopKPass top_k_pass_of(const TopKKeys& keys, uint32_t p) {
  uint32_t q = 0;
  for (uint32_t x = 1; x < keys.n && x < kTopKMaxKeys; x++)
    if (p >= keys.key[x].first) q = x;
  return {q, p - keys.key[q].first};
}
// The select's passes: bytes 0 .. len - 1, most significant first.  The sort's: the same bytes backwards.
inline std::vector<TopKPass> top_k_select_passes(const TopKKeys& keys) {
  std::vector<TopKPass> out;
  for (uint32_t p = 0; p < keys.len; p++) out.push_back(top_k_pass_of(keys, p));
  return out;
}
inline std::vector<TopKPass> top_k_sort_passes(const TopKKeys& keys) {
  std::vector<TopKPass> out = top_k_select_passes(keys);
  std::reverse(out.begin(), out.end());
  return out;
}

inline uint32_t top_k_stride(uint32_t len) { return (len + 7u) & ~7u; }

// ---- the workspace: behind the filter's, in the same allocation ----
// [o_state, + zero_bytes) is zeroed on the stream in front of every call.  What the one wait fetches beside the filter's counters:
// the state, and cap records at o_recs.
struct TopKWorkspace {
  uint64_t n_words = 0;
  uint32_t cap = 0;           // winners at most: min(k, n_in)
  uint32_t stride = 0;        // bytes from a key record to the next
  uint32_t sel_blocks = 0;    // blocks of top_k_pass_kernel
  uint32_t sort_blocks = 0;   // blocks of a sort pass: tiles of kTopKSortTile winners
  uint64_t o_state = 0, zero_bytes = 0, o_cand = 0, o_win = 0, o_final = 0, o_tie_cnt = 0, o_tie_off = 0, o_tie_sums = 0, o_tie_total = 0;
  uint64_t o_hist = 0, o_sort_hist = 0, o_rows2 = 0, o_recs = 0, recs_bytes = 0, bytes = 0;
  TopKWorkspace(uint64_t filter_bytes, uint32_t len, uint32_t k, uint64_t n_in) {
    FilterBump t;
    t.off = filter_bytes;
    n_words = (n_in + 63) / 64;
    cap = (uint32_t)std::min<uint64_t>(k, n_in);
    stride = top_k_stride(len);
    sel_blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_words + 3) / 4, 1024));
    sort_blocks = std::max<uint32_t>(1, (cap + kTopKSortTile - 1) / kTopKSortTile);
    zero_bytes = sizeof(TopKState);
    o_state = t.take(zero_bytes + 16);
    o_cand = t.take(n_words * 8 + 16);
    o_win = t.take(n_words * 8 + 16);
    o_final = t.take(n_words * 8 + 16);
    o_tie_cnt = t.take(n_words * 4 + 16);
    o_tie_off = t.take(n_words * 8 + 16);
    o_tie_sums = t.take(((n_words + 2047) / 2048) * 8 + 16);
    o_tie_total = t.take(16);
    o_hist = t.take((uint64_t)sel_blocks * 256 * 4 + 16);
    o_sort_hist = t.take((uint64_t)sort_blocks * 256 * 4 + 16);
    o_rows2 = t.take(n_in * 4 + 16);  // (the sort's other row list; as long as the filter's own, so that a place below n_in is in bounds)
    recs_bytes = (uint64_t)cap * stride;
    o_recs = t.take(recs_bytes + 16);
    bytes = t.off;
  }
};

// ---- key records: the comparison and the merge ----
inline int top_k_compare(const uint8_t* a, const uint8_t* b, uint32_t len) { return memcmp(a, b, len); }

// A key's part of a record from a value, as top_k_digit leaves it (the host check's hand cases; the kernels write the records)
inline void top_k_put_key(uint8_t* rec, const TopKKey& k, bool valid, uint64_t hi, uint64_t lo) {
  for (uint32_t b = 0; b < k.bytes; b++) rec[k.first + b] = (uint8_t)top_k_key_byte(k, valid, hi, lo, b);
}
inline void top_k_put_i64(uint8_t* rec, const TopKKey& k, bool valid, int64_t v) { top_k_put_key(rec, k, valid, 0, top_k_image_i64(v)); }
inline void top_k_put_bool(uint8_t* rec, const TopKKey& k, bool valid, bool v) { top_k_put_key(rec, k, valid, 0, v ? 1 : 0); }
inline void top_k_put_f64(uint8_t* rec, const TopKKey& k, bool valid, double v) { top_k_put_key(rec, k, valid, 0, top_k_image_f64(v)); }
inline void top_k_put_dec128(uint8_t* rec, const TopKKey& k, bool valid, uint64_t hi, uint64_t lo) { top_k_put_key(rec, k, valid, top_k_image_dec_hi(hi), lo); }

// What a stripe handed out: n rows in sorted order, their records one behind the other
struct TopKStripe {
  std::vector<uint8_t> recs;
  uint64_t n = 0;
};
// The global answer over the stripes in hand-out order: positions[i] = the index of its i-th row in the concatenation of the rows
// handed out.  Ties: the earlier stripe, then the earlier position.  *n = min(k, rows handed out); cap < *n:
// ORCGPU_INVALID_ARGUMENT with *n set and nothing written.
inline int top_k_merge(const std::vector<TopKStripe>& stripes, uint32_t len, uint32_t k, uint64_t* positions, uint64_t cap, uint64_t* n) {
  const uint32_t stride = top_k_stride(len);
  uint64_t total = 0;
  for (const TopKStripe& s : stripes) total += std::min<uint64_t>(s.n, stride ? s.recs.size() / stride : 0);
  const uint64_t want = std::min<uint64_t>(k, total);
  if (n) *n = want;
  if (cap < want || (want && !positions)) return ORCGPU_INVALID_ARGUMENT;
  struct Head {
    const uint8_t* rec;
    size_t stripe;
    uint64_t at, base;
  };
  auto later = [len](const Head& a, const Head& b) {  // (a priority_queue hands out the LAST under its order)
    const int c = top_k_compare(a.rec, b.rec, len);
    return c ? c > 0 : a.stripe > b.stripe;
  };
  std::priority_queue<Head, std::vector<Head>, decltype(later)> heads(later);
  uint64_t base = 0;
  std::vector<uint64_t> rows(stripes.size());
  for (size_t s = 0; s < stripes.size(); s++) {
    rows[s] = std::min<uint64_t>(stripes[s].n, stride ? stripes[s].recs.size() / stride : 0);
    if (rows[s]) heads.push({stripes[s].recs.data(), s, 0, base});
    base += stripes[s].n;
  }
  for (uint64_t i = 0; i < want; i++) {
    Head h = heads.top();
    heads.pop();
    positions[i] = h.base + h.at;
    if (++h.at < rows[h.stripe]) {
      h.rec += stride;
      heads.push(h);
    }
  }
  return ORCGPU_OK;
}

}  // namespace orcgpu_host
