// orcgpu_predicate.inc -- predicate pushdown onto row groups, host only: row-group statistics (statistics.rs:60-200), Bloom
// filters (bloom_filter.rs), evaluate_predicate (row_group_filter.rs:50-620), RowSelection::from_row_group_filter
// (row_selection.rs:348-392).  The reader (orcgpu_reader.inc) turns the outcome into the row groups it reads.
#include "orcgpu_decimal.inc"
#include "orcgpu_like.inc"
namespace orcgpu_host {

// ColumnStatistics of one row group (statistics.rs:115-200): TryFrom picks the first typed message present
struct GroupStats {
  bool present = false;  // RowIndexEntry.statistics
  uint64_t number_of_values = 0;
  bool has_null = false;
  enum Kind { NONE, INTEGER, DOUBLE, STRING, BUCKET, DECIMAL, DATE, BINARY, TIMESTAMP, COLLECTION } kind = NONE;
  int64_t imin = 0, imax = 0;            // Integer, Date; Timestamp: the UTC pair
  double dmin = 0, dmax = 0;
  std::string smin, smax;                // String (bounds), Decimal
  bool exact_min = false, exact_max = false;
  uint64_t true_count = 0;
};
struct GroupBloom {
  uint32_t num_hash_functions = 3;
  std::vector<uint64_t> bitset;
};
struct ColumnGroups {
  std::vector<GroupStats> stats;
  std::vector<GroupBloom> blooms;  // as many as stats, or none
};

inline int64_t pb_zigzag(uint64_t v) { return (int64_t)(v >> 1) ^ -(int64_t)(v & 1); }

bool parse_group_stats(const uint8_t* p, uint64_t n, GroupStats& st) {
  st.present = true;
  PbReader r(p, n);
  PbField f;
  // (field numbers: format/orc_proto.proto ColumnStatistics and the messages it holds)
  struct Typed {
    GroupStats::Kind kind;
    const uint8_t* p;
    uint64_t n;
  };
  Typed typed[13] = {};
  bool have[13] = {};
  while (r.next(f)) {
    if (f.num == 1 && f.wt == 0) st.number_of_values = f.v;
    else if (f.num == 10 && f.wt == 0) st.has_null = f.v != 0;
    else if (f.wt == 2 && f.num >= 2 && f.num <= 12 && f.num != 10 && f.num != 11) {
      typed[f.num] = Typed{GroupStats::NONE, f.p, f.n};
      have[f.num] = true;
    }
  }
  if (!r.ok) return false;
  if (st.number_of_values == 0) return true;  // "type_statistics: None"
  // int, double, string, bucket, decimal, date, binary, timestamp, collection -- in that order
  static const int order[] = {2, 3, 4, 5, 6, 7, 8, 9, 12};
  for (int num : order) {
    if (!have[num]) continue;
    PbReader q(typed[num].p, typed[num].n);
    PbField g;
    switch (num) {
      case 2:
        st.kind = GroupStats::INTEGER;
        while (q.next(g)) {
          if (g.num == 1 && g.wt == 0) st.imin = pb_zigzag(g.v);
          else if (g.num == 2 && g.wt == 0) st.imax = pb_zigzag(g.v);
        }
        break;
      case 3:
        st.kind = GroupStats::DOUBLE;
        while (q.next(g)) {
          if (g.num == 1 && g.wt == 1) memcpy(&st.dmin, &g.v, 8);
          else if (g.num == 2 && g.wt == 1) memcpy(&st.dmax, &g.v, 8);
        }
        break;
      case 4: {
        st.kind = GroupStats::STRING;
        std::string mn, mx, lo, up;
        bool hmn = false, hmx = false;
        while (q.next(g)) {
          if (g.wt != 2) continue;
          if (g.num == 1) mn.assign((const char*)g.p, g.n), hmn = true;
          else if (g.num == 2) mx.assign((const char*)g.p, g.n), hmx = true;
          else if (g.num == 4) lo.assign((const char*)g.p, g.n);
          else if (g.num == 5) up.assign((const char*)g.p, g.n);
        }
        st.smin = hmn ? mn : lo;
        st.exact_min = hmn;
        st.smax = hmx ? mx : up;
        st.exact_max = hmx;
        break;
      }
      case 5:
        st.kind = GroupStats::BUCKET;
        {
          bool first = true;
          while (q.next(g)) {
            if (g.num != 1) continue;
            if (g.wt == 0 && first) st.true_count = g.v, first = false;
            else if (g.wt == 2 && first) {
              PbReader pk(g.p, g.n);
              uint64_t v;
              if (pk.varint(&v)) st.true_count = v, first = false;
            }
          }
        }
        break;
      case 6:
        st.kind = GroupStats::DECIMAL;
        while (q.next(g)) {
          if (g.wt != 2) continue;
          if (g.num == 1) st.smin.assign((const char*)g.p, g.n);
          else if (g.num == 2) st.smax.assign((const char*)g.p, g.n);
        }
        break;
      case 7:
        st.kind = GroupStats::DATE;
        while (q.next(g)) {
          if (g.num == 1 && g.wt == 0) st.imin = (int32_t)pb_zigzag(g.v);
          else if (g.num == 2 && g.wt == 0) st.imax = (int32_t)pb_zigzag(g.v);
        }
        break;
      case 8: st.kind = GroupStats::BINARY; break;
      case 9:
        st.kind = GroupStats::TIMESTAMP;
        while (q.next(g)) {
          if (g.num == 3 && g.wt == 0) st.imin = pb_zigzag(g.v);  // minimumUtc
          else if (g.num == 4 && g.wt == 0) st.imax = pb_zigzag(g.v);  // maximumUtc
        }
        break;
      default: st.kind = GroupStats::COLLECTION; break;
    }
    return q.ok;
  }
  return true;
}

bool parse_column_groups(const uint8_t* row_index, uint64_t row_index_len, const uint8_t* bloom, uint64_t bloom_len, ColumnGroups& out) {
  PbReader r(row_index, row_index_len);
  PbField f;
  while (r.next(f)) {
    if (f.num != 1 || f.wt != 2) continue;  // RowIndex.entry
    GroupStats st;
    PbReader q(f.p, f.n);
    PbField g;
    while (q.next(g))
      if (g.num == 2 && g.wt == 2 && !parse_group_stats(g.p, g.n, st)) return false;
    if (!q.ok) return false;
    out.stats.push_back(std::move(st));
  }
  if (!r.ok) return false;
  if (bloom && bloom_len) {
    std::vector<GroupBloom> blooms;
    PbReader b(bloom, bloom_len);
    while (b.next(f)) {
      if (f.num != 1 || f.wt != 2) continue;  // BloomFilterIndex.bloomFilter
      GroupBloom gb;
      uint32_t nh = 0;
      std::vector<uint64_t> bits;
      std::string utf8;
      bool has_utf8 = false;
      PbReader q(f.p, f.n);
      PbField g;
      while (q.next(g)) {
        if (g.num == 1 && g.wt == 0) nh = (uint32_t)g.v;
        else if (g.num == 2 && g.wt == 1) bits.push_back(g.v);
        else if (g.num == 2 && g.wt == 2)
          for (uint64_t k = 0; k + 8 <= g.n; k += 8) {
            uint64_t w;
            memcpy(&w, g.p + k, 8);
            bits.push_back(w);
          }
        else if (g.num == 3 && g.wt == 2) utf8.assign((const char*)g.p, g.n), has_utf8 = true;
      }
      if (!q.ok) return false;
      if (bits.empty() && !has_utf8) continue;  // BloomFilter::try_from_proto: None (filter_map drops it)
      if (bits.empty())
        for (size_t k = 0; k < utf8.size(); k += 8) {
          uint64_t w = 0;
          memcpy(&w, utf8.data() + k, std::min<size_t>(8, utf8.size() - k));
          bits.push_back(w);
        }
      gb.num_hash_functions = nh ? nh : 3;
      gb.bitset = std::move(bits);
      blooms.push_back(std::move(gb));
    }
    if (!b.ok) return false;
    if (blooms.size() == out.stats.size()) out.blooms = std::move(blooms);  // (the reference asserts the counts agree)
  }
  return true;
}

// bloom_filter.rs: Murmur3 x64 (the 64-bit half ORC uses), Thomas Wang's 64-bit integer hash, the k probes
uint64_t bloom_hash_bytes(const uint8_t* p, size_t n) {
  const uint64_t C1 = 0x87c37b91114253d5ull, C2 = 0x4cf5ad432745937full;
  uint64_t h1 = 104729;
  const size_t nblocks = n / 8;
  auto rotl = [](uint64_t v, int r) { return (v << r) | (v >> (64 - r)); };
  for (size_t i = 0; i < nblocks; i++) {
    uint64_t k1;
    memcpy(&k1, p + 8 * i, 8);
    k1 *= C1;
    k1 = rotl(k1, 31);
    k1 *= C2;
    h1 ^= k1;
    h1 = rotl(h1, 27);
    h1 = h1 * 5 + 1390208809ull;
  }
  const uint8_t* tail = p + 8 * nblocks;
  const size_t tn = n - 8 * nblocks;
  uint64_t k1 = 0;
  for (size_t i = tn; i-- > 0;) k1 ^= (uint64_t)tail[i] << (8 * i);
  if (tn) {
    k1 *= C1;
    k1 = rotl(k1, 31);
    k1 *= C2;
    h1 ^= k1;
  }
  h1 ^= (uint64_t)n;
  h1 ^= h1 >> 33;
  h1 *= 0xff51afd7ed558ccdull;
  h1 ^= h1 >> 33;
  h1 *= 0xc4ceb9fe1a85ec53ull;
  h1 ^= h1 >> 33;
  return h1;
}
uint64_t bloom_hash_long(int64_t value) {
  uint64_t key = (uint64_t)value;
  key = (~key) + (key << 21);
  key ^= (uint64_t)((int64_t)key >> 24);
  key = key + (key << 3) + (key << 8);
  key ^= (uint64_t)((int64_t)key >> 14);
  key = key + (key << 2) + (key << 4);
  key ^= (uint64_t)((int64_t)key >> 28);
  key = key + (key << 31);
  return key;
}
bool bloom_test(const GroupBloom& b, uint64_t hash64) {
  const uint64_t bit_count = (uint64_t)b.bitset.size() * 64;
  if (!bit_count) return true;
  const int32_t hash1 = (int32_t)(uint32_t)hash64, hash2 = (int32_t)(uint32_t)(hash64 >> 32);
  for (uint32_t i = 1; i <= b.num_hash_functions; i++) {
    int32_t combined = (int32_t)((uint32_t)hash1 + (uint32_t)i * (uint32_t)hash2);
    if (combined < 0) combined = ~combined;
    const uint64_t bit = (uint64_t)(uint32_t)combined % bit_count;
    if (!((b.bitset[bit / 64] >> (bit % 64)) & 1)) return false;
  }
  return true;
}

struct PredNode {
  int op = 0;
  uint32_t n_children = 0;
  std::string column;
  bool has_column = false;  // (the row filter tells a leaf without a name from one with an empty name)
  int value_type = 0;
  bool value_is_null = false;
  int64_t i = 0;
  double f = 0;
  std::string s;
};

struct PredEval {
  const std::vector<PredNode>& nodes;
  const std::vector<std::string>& names;
  const std::vector<ColumnGroups>& cols;
  size_t n_groups;
  bool failed = false;  // the reference's `?`: the whole evaluation is an Err
  // columns the statistics know nothing of (the reader's computed columns): a leaf on one is a sound "might match", under a NOT
  // too, and never fails the evaluation -- what it cannot take is the row filter's to report
  const std::vector<std::string>* opaque = nullptr;
  bool is_opaque(const PredNode& n) const {
    if (!opaque || !n.has_column) return false;
    for (const std::string& o : *opaque)
      if (o == n.column) return true;
    return false;
  }

  static int negate(int op) {  // ComparisonOp::negate
    switch (op) {
      case ORCGPU_PRED_EQ: return ORCGPU_PRED_NE;
      case ORCGPU_PRED_NE: return ORCGPU_PRED_EQ;
      case ORCGPU_PRED_LT: return ORCGPU_PRED_GE;
      case ORCGPU_PRED_LE: return ORCGPU_PRED_GT;
      case ORCGPU_PRED_GT: return ORCGPU_PRED_LE;
      default: return ORCGPU_PRED_LT;
    }
  }
  const ColumnGroups* column(const std::string& name) {
    for (size_t k = 0; k < names.size(); k++)
      if (names[k] == name) return &cols[k];
    failed = true;  // "Column not found in schema" / "Row index not found for column"
    return nullptr;
  }
  static bool cmp_int(int64_t min, int64_t max, int op, int64_t v) {
    switch (op) {
      case ORCGPU_PRED_EQ: return min <= v && v <= max;
      case ORCGPU_PRED_NE: return !(min == v && max == v);
      case ORCGPU_PRED_LT: return min < v;
      case ORCGPU_PRED_LE: return min <= v;
      case ORCGPU_PRED_GT: return max > v;
      default: return max >= v;
    }
  }
  static bool cmp_float(double min, double max, int op, double v) {
    const double eps = 1e-9;
    switch (op) {
      case ORCGPU_PRED_EQ: return (min - eps) <= v && v <= (max + eps);
      case ORCGPU_PRED_NE: return !(std::fabs(min - v) < eps && std::fabs(max - v) < eps);
      case ORCGPU_PRED_LT: return min < v;
      case ORCGPU_PRED_LE: return min <= v;
      case ORCGPU_PRED_GT: return max > v;
      default: return max >= v;
    }
  }
  static bool cmp_string(const std::string& lo, const std::string& up, int op, const std::string& v, bool exact_min, bool exact_max) {
    const bool min_le = lo < v || (lo == v && exact_min), max_ge = up > v || (up == v && exact_max);
    switch (op) {
      case ORCGPU_PRED_EQ: return min_le && max_ge;
      case ORCGPU_PRED_LE: return min_le;
      case ORCGPU_PRED_GE: return max_ge;
      case ORCGPU_PRED_LT: return lo < v;
      case ORCGPU_PRED_GT: return up > v;
      default: return !(lo == up && exact_min && exact_max && lo == v);
    }
  }
  // evaluate_comparison_with_stats (row_group_filter.rs:195-330)
  bool stats_match(const GroupStats& st, int op, const PredNode& n) {
    const bool some = !n.value_is_null;
    const int vt = n.value_type;
    const bool is_int = some && vt >= ORCGPU_PV_INT8 && vt <= ORCGPU_PV_INT64;
    switch (st.kind) {
      case GroupStats::NONE: failed = true; return true;  // "Statistics missing type-specific information"
      case GroupStats::INTEGER:
        if (!is_int) return failed = true;
        return cmp_int(st.imin, st.imax, op, n.i);
      case GroupStats::DOUBLE:
        if (!(some && (vt == ORCGPU_PV_FLOAT32 || vt == ORCGPU_PV_FLOAT64))) return failed = true;
        return cmp_float(st.dmin, st.dmax, op, vt == ORCGPU_PV_FLOAT32 ? (double)(float)n.f : n.f);
      case GroupStats::STRING:
        if (!(some && vt == ORCGPU_PV_UTF8)) return failed = true;
        return cmp_string(st.smin, st.smax, op, n.s, st.exact_min, st.exact_max);
      case GroupStats::DATE:
        if (!(some && (vt == ORCGPU_PV_INT32 || vt == ORCGPU_PV_INT64))) return failed = true;
        return cmp_int(st.imin, st.imax, op, n.i);
      case GroupStats::TIMESTAMP:
        // (a TimestampNs literal prunes nothing and fails nothing: the statistics are UTC milliseconds, and what a non-instant
        // column exports depends on the writer's time zone, which this rule does not have)
        if (vt == ORCGPU_PV_TIMESTAMP_NS) return true;
        if (!(some && vt == ORCGPU_PV_INT64)) return failed = true;
        return cmp_int(st.imin, st.imax, op, n.i);
      case GroupStats::DECIMAL:
        if (some && vt == ORCGPU_PV_DECIMAL128) {  // exact rational order (the reference has no such literal)
          i128 v;
          bool m = true;
          if (!dec_literal(n.s.data(), n.s.size(), n.i, v) || !dec_stats_match(st.smin, st.smax, op, v, (int)n.i, &m)) return failed = true;
          return m;
        }
        // (a Utf8 literal: compared as strings, as the reference does)
        if (!(some && vt == ORCGPU_PV_UTF8)) return failed = true;
        return cmp_string(st.smin, st.smax, op, n.s, true, true);
      case GroupStats::BUCKET: {
        if (!(some && vt == ORCGPU_PV_BOOLEAN)) return failed = true;
        const uint64_t t = st.true_count, fcount = st.number_of_values - t;
        const bool v = n.i != 0;
        if (op == ORCGPU_PRED_EQ) return v ? t > 0 : fcount > 0;
        if (op == ORCGPU_PRED_NE) return v ? fcount > 0 : t > 0;
        return true;
      }
      default: return true;  // Binary, Collection
    }
  }
  // row_group_might_match_bloom (row_group_filter.rs:332-371)
  static bool bloom_match(const GroupBloom* b, int op, const PredNode& n) {
    if (op != ORCGPU_PRED_EQ || !b || n.value_is_null) return true;
    uint64_t h;
    switch (n.value_type) {
      case ORCGPU_PV_UTF8: h = bloom_hash_bytes((const uint8_t*)n.s.data(), n.s.size()); break;
      case ORCGPU_PV_INT8: case ORCGPU_PV_INT16: case ORCGPU_PV_INT32: case ORCGPU_PV_INT64: h = bloom_hash_long(n.i); break;
      case ORCGPU_PV_FLOAT32: case ORCGPU_PV_FLOAT64: {
        const double d = n.value_type == ORCGPU_PV_FLOAT32 ? (double)(float)n.f : n.f;
        int64_t bits;
        memcpy(&bits, &d, 8);
        h = bloom_hash_long(bits);
        break;
      }
      case ORCGPU_PV_BOOLEAN: h = bloom_hash_long(n.i ? 1 : 0); break;
      default: return true;
    }
    return bloom_test(*b, h);
  }
  void comparison(const PredNode& n, int op, std::vector<uint8_t>& result) {
    const ColumnGroups* c = column(n.column);
    if (!c) return;
    for (size_t g = 0; g < result.size() && g < c->stats.size(); g++) {
      const GroupStats& st = c->stats[g];
      bool m = st.present ? stats_match(st, op, n) : true;
      if (failed) return;
      if (!m) {
        result[g] = 0;
        continue;
      }
      result[g] = bloom_match(c->blooms.empty() ? nullptr : &c->blooms[g], op, n) ? 1 : 0;
    }
  }
  void null_test(const PredNode& n, bool is_null, std::vector<uint8_t>& result) {
    const ColumnGroups* c = column(n.column);
    if (!c) return;
    for (size_t g = 0; g < result.size() && g < c->stats.size(); g++) {
      const GroupStats& st = c->stats[g];
      result[g] = !st.present ? 1 : (is_null ? st.has_null : st.number_of_values > 0);
    }
  }
  // A LIKE leaf (ORCGPU_PRED_LIKE; the reference has none) is a sound "might match" and never fails the evaluation -- a malformed
  // pattern is the row filter's to report.  Not under a NOT, on String statistics: a pattern without a wildcard is EQ on its
  // unescaped bytes, Bloom filter included; one with the literal prefix p in front of its first wildcard can only match values in
  // [p, succ(p)), so the group is kept iff its upper bound >= p and its lower bound < succ(p) (truncated bounds are still bounds;
  // p all 0xFF: the first test alone).  Everything else keeps every group.
  void like(const PredNode& n, bool neg, std::vector<uint8_t>& result) {
    if (neg || n.value_is_null || n.value_type != ORCGPU_PV_UTF8 || n.i < 0 || n.i > 127) return;
    const ColumnGroups* c = nullptr;
    for (size_t k = 0; k < names.size() && !c; k++)
      if (names[k] == n.column) c = &cols[k];
    LikePattern pat;
    if (!c || !like_unescape(n.s.data(), n.s.size(), (int)n.i, pat)) return;
    const bool exact = pat.wildcard_free();
    const std::string p = pat.prefix();
    if (!exact && p.empty()) return;
    std::string succ;
    const bool has_succ = like_prefix_succ(p, succ);
    PredNode lit = n;  // (what the EQ rule and the Bloom filter are asked)
    lit.s = p;
    for (size_t g = 0; g < result.size() && g < c->stats.size(); g++) {
      const GroupStats& st = c->stats[g];
      const bool strings = st.present && st.kind == GroupStats::STRING;
      if (st.present && !strings) continue;
      if (exact) {
        if (strings && !cmp_string(st.smin, st.smax, ORCGPU_PRED_EQ, p, st.exact_min, st.exact_max)) result[g] = 0;
        else if (!bloom_match(c->blooms.empty() ? nullptr : &c->blooms[g], ORCGPU_PRED_EQ, lit)) result[g] = 0;
      } else if (strings && (st.smax < p || (has_succ && !(st.smin < succ)))) result[g] = 0;
    }
  }
  // An IN leaf (ORCGPU_PRED_IN; the reference has none) keeps the groups the OR of its EQ leaves keeps, by the rules of
  // comparison() per literal: statistics, then the Bloom filter; a literal of the wrong type and a group without typed statistics
  // fail the evaluation as they do for EQ.  One difference: Double statistics whose minimum or maximum is a NaN bound nothing, and
  // the group is kept.  Under a NOT every group is kept (sound; NE's rule buys nothing for a list).  The
  // literals are sorted once per leaf and the ones inside a group's [min, max] are found by binary search; only those are put to
  // the Bloom filter, so 65536 literals do not cost 65536 tests per group.
  void in_list(size_t at, bool neg, std::vector<uint8_t>& result) {
    const PredNode& n = nodes[at];
    const size_t k = n.n_children;
    for (size_t x = 0; x < k; x++)
      if (nodes[at + 1 + x].op != ORCGPU_PRED_LITERAL) {
        failed = true;
        return;
      }
    if (neg) return;
    if (!k) {  // an OR of no children: no group can hold a row
      std::fill(result.begin(), result.end(), 0);
      return;
    }
    const ColumnGroups* c = column(n.column);
    if (!c) return;
    // the literals by kind, each kind in the order its statistics compare in; .second = the literal's node
    std::vector<std::pair<int64_t, size_t>> ints;
    std::vector<std::pair<double, size_t>> floats;
    std::vector<std::pair<std::string, size_t>> strs;
    struct Dec {
      i128 v;
      int scale;
      size_t node;
    };
    std::vector<Dec> decs;
    size_t n_i8_16 = 0, n_bool = 0, n_ts = 0, n_nan = 0, n_bad_dec = 0;
    bool has_true = false, has_false = false;
    size_t node_true = 0, node_false = 0;
    for (size_t x = 0; x < k; x++) {
      const PredNode& l = nodes[at + 1 + x];
      const int vt = l.value_type;
      n_ts += vt == ORCGPU_PV_TIMESTAMP_NS;  // (the NULL one as well: Timestamp statistics take it as it is)
      if (l.value_is_null) continue;
      if (vt >= ORCGPU_PV_INT8 && vt <= ORCGPU_PV_INT64) {
        ints.emplace_back(l.i, at + 1 + x);
        n_i8_16 += vt == ORCGPU_PV_INT8 || vt == ORCGPU_PV_INT16;
      } else if (vt == ORCGPU_PV_FLOAT32 || vt == ORCGPU_PV_FLOAT64) {
        const double d = vt == ORCGPU_PV_FLOAT32 ? (double)(float)l.f : l.f;
        if (d == d) floats.emplace_back(d, at + 1 + x);
        else n_nan++;  // (inside no [min - eps, max + eps])
      } else if (vt == ORCGPU_PV_UTF8) strs.emplace_back(l.s, at + 1 + x);
      else if (vt == ORCGPU_PV_BOOLEAN) {
        n_bool++;
        if (l.i) has_true = true, node_true = at + 1 + x;
        else has_false = true, node_false = at + 1 + x;
      } else if (vt == ORCGPU_PV_DECIMAL128) {
        Dec d{0, (int)l.i, at + 1 + x};
        if (dec_literal(l.s.data(), l.s.size(), l.i, d.v)) decs.push_back(d);
        else n_bad_dec++;
      }
    }
    const size_t n_float = floats.size() + n_nan, n_dec = decs.size() + n_bad_dec;
    std::sort(ints.begin(), ints.end());
    std::sort(floats.begin(), floats.end());
    std::sort(strs.begin(), strs.end());
    std::sort(decs.begin(), decs.end(), [](const Dec& a, const Dec& b) { return dec_cmp(a.v, a.scale, b.v, b.scale) < 0; });
    std::vector<uint8_t> any(result.size(), 0);
    for (size_t g = 0; g < result.size() && g < c->stats.size(); g++) {
      const GroupStats& st = c->stats[g];
      const GroupBloom* bloom = c->blooms.empty() ? nullptr : &c->blooms[g];
      auto ask = [&](size_t node) { return bloom_match(bloom, ORCGPU_PRED_EQ, nodes[node]); };
      bool keep = false;
      if (!st.present) {  // no statistics: every literal is inside, the Bloom filter alone can say no
        for (size_t x = 0; x < k && !keep; x++) keep = ask(at + 1 + x);
        any[g] = keep;
        continue;
      }
      switch (st.kind) {
        case GroupStats::NONE:
          failed = true;
          return;
        case GroupStats::INTEGER: case GroupStats::DATE: case GroupStats::TIMESTAMP: {
          if (st.kind == GroupStats::TIMESTAMP) {
            // (a TimestampNs literal prunes nothing and fails nothing; any other literal must be an Int64)
            if (ints.size() + n_ts != k || n_i8_16) return (void)(failed = true);
            for (auto& e : ints)
              if (nodes[e.second].value_type != ORCGPU_PV_INT64) return (void)(failed = true);
            if (n_ts) {
              keep = true;
              break;
            }
          } else if (ints.size() != k || (st.kind == GroupStats::DATE && n_i8_16)) return (void)(failed = true);
          auto lo = std::lower_bound(ints.begin(), ints.end(), std::make_pair(st.imin, (size_t)0));
          for (; lo != ints.end() && lo->first <= st.imax && !keep; ++lo) keep = ask(lo->second);
          break;
        }
        case GroupStats::DOUBLE: {
          if (n_float != k) return (void)(failed = true);
          const double eps = 1e-9;
          if (st.dmin != st.dmin || st.dmax != st.dmax) {
            // (a NaN in the group has poisoned the writer's minimum / maximum: they bound nothing, so every literal is inside.
            // EQ's own rule, the reference's, finds nothing inside such a pair; a list is not made unsound for its sake)
            for (size_t x = 0; x < floats.size() && !keep; x++) keep = ask(floats[x].second);
            break;
          }
          auto lo = std::lower_bound(floats.begin(), floats.end(), std::make_pair(st.dmin - eps, (size_t)0));
          for (; lo != floats.end() && lo->first <= st.dmax + eps && !keep; ++lo) keep = ask(lo->second);
          break;
        }
        case GroupStats::STRING: case GroupStats::DECIMAL: {
          const bool is_dec = st.kind == GroupStats::DECIMAL;
          if (strs.size() + (is_dec ? n_dec : 0) != k || n_bad_dec) return (void)(failed = true);
          // (the strings from the lower bound on, each by EQ's own rule: exact and truncated bounds differ at the ends only)
          auto lo = std::lower_bound(strs.begin(), strs.end(), st.smin, [](const std::pair<std::string, size_t>& e, const std::string& v) { return e.first < v; });
          for (; lo != strs.end() && !(st.smax < lo->first) && !keep; ++lo)
            keep = cmp_string(st.smin, st.smax, ORCGPU_PRED_EQ, lo->first, is_dec || st.exact_min, is_dec || st.exact_max) && ask(lo->second);
          if (is_dec && !decs.empty()) {
            i128 mn, mx;
            int mn_scale, mx_scale;
            if (!dec_parse(st.smin, mn, mn_scale) || !dec_parse(st.smax, mx, mx_scale)) return (void)(failed = true);
            auto dl = std::lower_bound(decs.begin(), decs.end(), 0, [&](const Dec& e, int) { return dec_cmp(e.v, e.scale, mn, mn_scale) < 0; });
            for (; dl != decs.end() && dec_cmp(dl->v, dl->scale, mx, mx_scale) <= 0 && !keep; ++dl) keep = ask(dl->node);
          }
          break;
        }
        case GroupStats::BUCKET: {
          if (n_bool != k) return (void)(failed = true);
          const uint64_t t = st.true_count, fcount = st.number_of_values - t;
          keep = (has_true && t > 0 && ask(node_true)) || (has_false && fcount > 0 && ask(node_false));
          break;
        }
        default:  // Binary, Collection: the statistics say nothing, whatever the literal
          for (size_t x = 0; x < k && !keep; x++) keep = ask(at + 1 + x);
          break;
      }
      any[g] = keep;
    }
    for (size_t g = 0; g < result.size(); g++) result[g] = g < c->stats.size() ? any[g] : result[g];
  }
  // the index behind the expression subtree at `at` (ORCGPU_PRED_EXPR_* nodes with their own child counts), or 0 for what is none
  size_t expr_end(size_t at) const {
    if (at >= nodes.size()) return 0;
    const PredNode& n = nodes[at];
    const uint32_t kids = n.op == ORCGPU_PRED_EXPR_COLUMN || n.op == ORCGPU_PRED_EXPR_LITERAL ? 0 : n.op == ORCGPU_PRED_EXPR_NEG || n.op == ORCGPU_PRED_EXPR_DATE_PART ? 1
                        : n.op == ORCGPU_PRED_EXPR_ADD || n.op == ORCGPU_PRED_EXPR_SUB || n.op == ORCGPU_PRED_EXPR_MUL ? 2
                        : n.op == ORCGPU_PRED_EXPR_DIV || n.op == ORCGPU_PRED_EXPR_FLOOR_DIV || n.op == ORCGPU_PRED_EXPR_MOD ? 2  // (never pruned through: a leaf that holds one has no bare column beside one literal)
                        // ... and the conditionals, never pruned through for the same reason
                        : n.op == ORCGPU_PRED_EXPR_IF ? 3 : n.op == ORCGPU_PRED_EXPR_NULL ? 0
                        : n.op == ORCGPU_PRED_EXPR_ABS || n.op == ORCGPU_PRED_EXPR_IS_NULL || n.op == ORCGPU_PRED_EXPR_NOT ? 1
                        : n.op >= ORCGPU_PRED_EXPR_CAST && n.op <= ORCGPU_PRED_EXPR_TRUNC ? 1  // (the conversions: never pruned through either)
                        : n.op == ORCGPU_PRED_EXPR_COALESCE || n.op == ORCGPU_PRED_EXPR_CMP || n.op == ORCGPU_PRED_EXPR_AND || n.op == ORCGPU_PRED_EXPR_OR ? 2 : ~0u;
    if (kids == ~0u || n.n_children != kids) return 0;
    size_t next = at + 1;
    for (uint32_t k = 0; k < kids; k++)
      if (!(next = expr_end(next))) return 0;
    return next;
  }
  // An expression leaf (ORCGPU_PRED_CMP_EXPR; the reference has none) is a sound "might match" and never fails the evaluation:
  // what it cannot take is the row filter's to report.  One form prunes: a bare column against ONE literal node is the comparison
  // it equals, the operator mirrored when the column stands on the right, by the rules of comparison() -- where those rules would
  // fail the evaluation (an INT64 literal beside Decimal statistics, a column without an index) every group is kept instead.
  // Returns the index behind the leaf; a malformed one fails the evaluation like any malformed node list.
  size_t cmp_expr(size_t at, bool neg, std::vector<uint8_t>& result) {
    const PredNode& n = nodes[at];
    const size_t l = at + 1, r = n.n_children == 2 ? expr_end(l) : 0, end = r ? expr_end(r) : 0;
    if (!end || n.i < ORCGPU_PRED_EQ || n.i > ORCGPU_PRED_GE) {
      failed = true;
      return nodes.size();
    }
    const bool col_left = nodes[l].op == ORCGPU_PRED_EXPR_COLUMN && nodes[r].op == ORCGPU_PRED_EXPR_LITERAL;
    const bool col_right = nodes[l].op == ORCGPU_PRED_EXPR_LITERAL && nodes[r].op == ORCGPU_PRED_EXPR_COLUMN;
    if ((!col_left && !col_right) || failed) return end;
    int op = (int)n.i;
    if (col_right) op = op == ORCGPU_PRED_LT ? ORCGPU_PRED_GT : op == ORCGPU_PRED_GT ? ORCGPU_PRED_LT : op == ORCGPU_PRED_LE ? ORCGPU_PRED_GE : op == ORCGPU_PRED_GE ? ORCGPU_PRED_LE : op;
    PredNode leaf = nodes[col_left ? r : l];  // the literal, as the comparison node it stands for
    leaf.op = op;
    leaf.n_children = 0;
    leaf.column = nodes[col_left ? l : r].column;
    leaf.has_column = true;
    std::vector<uint8_t> t = result;
    comparison(leaf, neg ? negate(op) : op, t);
    if (failed) failed = false;  // (kept whole)
    else result = t;
    return end;
  }
  // one subtree in pre-order; returns the index behind it.  `neg`: under a NOT (pushed down as the reference does)
  size_t eval(size_t at, bool neg, std::vector<uint8_t>& result) {
    if (at >= nodes.size() || failed) {
      failed = true;
      return nodes.size();
    }
    const PredNode& n = nodes[at];
    if (is_opaque(n) && (n.op <= ORCGPU_PRED_GE || n.op == ORCGPU_PRED_IS_NULL || n.op == ORCGPU_PRED_IS_NOT_NULL || n.op == ORCGPU_PRED_LIKE)) return at + 1;
    if (is_opaque(n) && n.op == ORCGPU_PRED_IN && at + 1 + (size_t)n.n_children <= nodes.size()) return at + 1 + n.n_children;
    if (n.op == ORCGPU_PRED_IN) {
      if (at + 1 + (size_t)n.n_children > nodes.size()) {
        failed = true;
        return nodes.size();
      }
      in_list(at, neg, result);
      return at + 1 + n.n_children;
    }
    if (n.op == ORCGPU_PRED_LIKE) {
      like(n, neg, result);
      return at + 1;
    }
    if (n.op == ORCGPU_PRED_CMP_EXPR) return cmp_expr(at, neg, result);
    // A set leaf (ORCGPU_PRED_IN_SET) is a sound "might match": the set's keys live on the device, so every group is kept, under
    // a NOT too, and the evaluation never fails on it -- what the leaf cannot take is the row filter's to report.
    if (n.op == ORCGPU_PRED_IN_SET) return at + 1;
    if (n.op <= ORCGPU_PRED_GE) {
      comparison(n, neg ? negate(n.op) : n.op, result);
      return at + 1;
    }
    if (n.op == ORCGPU_PRED_IS_NULL || n.op == ORCGPU_PRED_IS_NOT_NULL) {
      null_test(n, (n.op == ORCGPU_PRED_IS_NULL) != neg, result);
      return at + 1;
    }
    if (n.op == ORCGPU_PRED_NOT) return eval(at + 1, !neg, result);
    if (n.op != ORCGPU_PRED_AND && n.op != ORCGPU_PRED_OR) {
      failed = true;
      return nodes.size();
    }
    // And: result &= every child (each from all-true); Or: result = any child.  De Morgan under a NOT
    const bool conj = (n.op == ORCGPU_PRED_AND) != neg;
    std::vector<uint8_t> any(result.size(), 0);
    size_t next = at + 1;
    for (uint32_t k = 0; k < n.n_children && !failed; k++) {
      std::vector<uint8_t> t(result.size(), 1);
      next = eval(next, neg, t);
      for (size_t g = 0; g < result.size(); g++) {
        if (conj) result[g] = result[g] && t[g];
        else any[g] = any[g] || t[g];
      }
    }
    if (!conj)
      for (size_t g = 0; g < result.size(); g++) result[g] = any[g];
    return next;
  }
};

std::vector<PredNode> copy_predicate(const orcgpu_predicate_node* nodes, uint32_t n) {
  std::vector<PredNode> out(n);
  for (uint32_t k = 0; k < n; k++) {
    out[k].op = nodes[k].op;
    out[k].n_children = nodes[k].n_children;
    if (nodes[k].column) out[k].column = nodes[k].column;
    out[k].has_column = nodes[k].column != nullptr;
    out[k].value_type = nodes[k].value_type;
    out[k].value_is_null = nodes[k].value_is_null != 0;
    out[k].i = nodes[k].i;
    out[k].f = nodes[k].f;
    if (nodes[k].s) out[k].s.assign(nodes[k].s, (size_t)nodes[k].s_len);
  }
  return out;
}
// ... and back: the nodes as the C ABI spells them, viewing the strings of `nodes` (which must outlive the view)
std::vector<orcgpu_predicate_node> view_predicate(const std::vector<PredNode>& nodes) {
  std::vector<orcgpu_predicate_node> out(nodes.size());
  for (size_t k = 0; k < nodes.size(); k++) {
    const PredNode& p = nodes[k];
    orcgpu_predicate_node& n = out[k];
    memset(&n, 0, sizeof(n));
    n.op = p.op;
    n.n_children = p.n_children;
    n.column = p.has_column ? p.column.c_str() : nullptr;
    n.value_type = p.value_type;
    n.value_is_null = p.value_is_null ? 1 : 0;
    n.i = p.i;
    n.f = p.f;
    n.s = p.s.data();
    n.s_len = p.s.size();
  }
  return out;
}

// evaluate_predicate: false = the evaluation is an Err (the reader then selects every row of the stripe)
bool predicate_row_groups(const std::vector<PredNode>& nodes, const std::vector<std::string>& names, const std::vector<ColumnGroups>& cols,
                          size_t n_groups, std::vector<uint8_t>& keep, const std::vector<std::string>* opaque = nullptr) {
  keep.assign(n_groups, 1);
  PredEval ev{nodes, names, cols, n_groups};
  ev.opaque = opaque;
  const size_t end = ev.eval(0, false, keep);
  return !ev.failed && end == nodes.size();
}

}  // namespace orcgpu_host

extern "C" int orcgpu_predicate_row_groups(const orcgpu_predicate_node* nodes, uint32_t n_nodes, const orcgpu_column_index* columns, uint32_t n_columns,
                                           uint64_t stripe_rows, uint64_t rows_per_group, uint8_t* keep, uint32_t* n_groups) {
  if (!nodes || !n_nodes || (n_columns && !columns) || !keep || !n_groups) return ORCGPU_INVALID_ARGUMENT;
  const uint64_t ng = rows_per_group ? (stripe_rows + rows_per_group - 1) / rows_per_group : 0;
  *n_groups = (uint32_t)ng;
  std::vector<std::string> names;
  std::vector<orcgpu_host::ColumnGroups> cols;
  for (uint32_t k = 0; k < n_columns; k++) {
    if (!columns[k].row_index) continue;  // (no ROW_INDEX stream: "Row index not found for column")
    orcgpu_host::ColumnGroups cg;
    if (!orcgpu_host::parse_column_groups(columns[k].row_index, columns[k].row_index_len, columns[k].bloom_index, columns[k].bloom_index_len, cg))
      return ORCGPU_OUT_OF_SPEC;
    names.emplace_back(columns[k].name ? columns[k].name : "");
    cols.push_back(std::move(cg));
  }
  std::vector<uint8_t> out;
  if (!orcgpu_host::predicate_row_groups(orcgpu_host::copy_predicate(nodes, n_nodes), names, cols, (size_t)ng, out)) return ORCGPU_UNEXPECTED;
  for (uint64_t g = 0; g < ng; g++) keep[g] = out[g];
  return ORCGPU_OK;
}
