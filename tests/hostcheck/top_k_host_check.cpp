// top_k_host_check.cpp -- the host side of ORDER BY ... LIMIT k (orc_rust_amd/csrc/orcgpu_top_k_host.inc and device/top_k_program.h,
// the very text liborcgpu.so is built from) under AddressSanitizer + UBSan, on the CPU (TEST INFRASTRUCTURE).  A stand-alone
// program: it builds its cases itself and prints one line per fact, "<name> <values ...>[\t<message>]";
// tests/test_top_k_host_sanitized.py holds the lines to what include/orcgpu.h says.  Exit code 0 when it ran through; a sanitizer
// report aborts with its own exit code.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/orcgpu.h"
#include "../../orc_rust_amd/csrc/orcgpu_filter_host.inc"
#include "../../orc_rust_amd/csrc/orcgpu_agg_plan.inc"
#include "../../orc_rust_amd/csrc/orcgpu_top_k_host.inc"

using namespace orcgpu_host;

static AggCol col(int32_t orc_type, uint32_t width, bool dict = false, int32_t ts_unit = 3, bool nested = false) {
  AggCol a;
  a.d.orc_type = orc_type;
  a.d.width = width;
  a.d.ts_unit = ts_unit;
  a.d.is_bool = orc_type == ORCGPU_T_BOOLEAN;
  a.d.dict_out = dict;
  a.d.is_string = !dict && (orc_type == ORCGPU_T_STRING || orc_type == ORCGPU_T_BINARY);
  a.d.has_present = true;
  a.nested = nested;
  return a;
}
static const char* const kNames[] = {"i64", "f32", "b", "dec", "s", "dict", "ts_ns", "ts_dec", "bin", "date", "i8"};
static const AggCol kCols[] = {col(ORCGPU_T_LONG, 8),   col(ORCGPU_T_FLOAT, 4),        col(ORCGPU_T_BOOLEAN, 0),        col(ORCGPU_T_DECIMAL, 16),
                               col(ORCGPU_T_STRING, 0), col(ORCGPU_T_STRING, 4, true), col(ORCGPU_T_TIMESTAMP, 8, false, 3), col(ORCGPU_T_TIMESTAMP, 16, false, 4),
                               col(ORCGPU_T_BINARY, 0), col(ORCGPU_T_DATE, 4),         col(ORCGPU_T_BYTE, 1)};
static const uint32_t kNc = 11;

static orcgpu_sort_key key(const char* c, uint32_t desc = 0, uint32_t nf = 0) { return {c, desc, nf}; }

static void show_plan(const char* name, std::vector<orcgpu_sort_key> keys, uint32_t k = 10) {
  TopKPlan plan;
  const int rc = top_k_compile(keys.data(), (uint32_t)keys.size(), k, kNames, kCols, kNc, plan);
  printf("%s %d", name, rc);
  if (!rc) {
    printf(" %u %u", plan.keys.n, plan.keys.len);
    for (uint32_t q = 0; q < plan.keys.n; q++) {
      const TopKKey& x = plan.keys.key[q];
      printf(" %u:%u:%u:%u:%u:%u", x.col, x.kind, x.descending, x.nulls_first, x.first, x.bytes);
    }
  }
  printf("\t%s\n", plan.err);
}
static void show_passes(const char* name, std::vector<orcgpu_sort_key> keys) {
  TopKPlan plan;
  if (top_k_compile(keys.data(), (uint32_t)keys.size(), 1, kNames, kCols, kNc, plan)) return;
  const std::vector<TopKPass> sel = top_k_select_passes(plan.keys), srt = top_k_sort_passes(plan.keys);
  printf("%s_select %zu", name, sel.size());
  for (const TopKPass& p : sel) printf(" %u.%u", p.key, p.byte);
  printf("\n%s_sort %zu", name, srt.size());
  for (const TopKPass& p : srt) printf(" %u.%u", p.key, p.byte);
  printf("\n");
}

static void show_workspace(const char* name, uint64_t filter_bytes, uint32_t len, uint32_t k, uint64_t n_in) {
  const TopKWorkspace w(filter_bytes, len, k, n_in);
  struct Piece {
    uint64_t off, bytes;
  };
  const Piece pieces[] = {{w.o_state, w.zero_bytes},
                          {w.o_cand, w.n_words * 8},
                          {w.o_win, w.n_words * 8},
                          {w.o_final, w.n_words * 8},
                          {w.o_tie_cnt, w.n_words * 4},
                          {w.o_tie_off, w.n_words * 8},
                          {w.o_tie_sums, (w.n_words + 2047) / 2048 * 8},
                          {w.o_tie_total, 16},
                          {w.o_hist, (uint64_t)w.sel_blocks * 1024},
                          {w.o_sort_hist, (uint64_t)w.sort_blocks * 1024},
                          {w.o_rows2, n_in * 4},
                          {w.o_recs, w.recs_bytes}};
  bool aligned = true, ordered = true;
  uint64_t end = filter_bytes;
  for (const Piece& p : pieces) {
    aligned = aligned && p.off % kFilterAlign == 0;
    ordered = ordered && p.off >= end;
    end = p.off + p.bytes;
  }
  printf("%s %d %d %d %u %u %u %u %llu\n", name, aligned, ordered, end <= w.bytes, w.cap, w.stride, w.sel_blocks, w.sort_blocks, (unsigned long long)w.recs_bytes);
}

// ---- records of hand cases: one key, value v, and their order by top_k_compare ----
struct Val {
  bool valid;
  double f;
  int64_t i;
  uint64_t hi, lo;
};
static std::vector<size_t> order_of(const TopKKey& k, const std::vector<Val>& vals, int kind) {
  const uint32_t len = k.bytes, stride = top_k_stride(len);
  std::vector<uint8_t> recs(vals.size() * stride, 0);
  for (size_t x = 0; x < vals.size(); x++) {
    uint8_t* r = recs.data() + x * stride;
    if (kind == TK_FLOAT) top_k_put_f64(r, k, vals[x].valid, vals[x].f);
    else if (kind == TK_INT) top_k_put_i64(r, k, vals[x].valid, vals[x].i);
    else if (kind == TK_BOOL) top_k_put_bool(r, k, vals[x].valid, vals[x].i != 0);
    else top_k_put_dec128(r, k, vals[x].valid, vals[x].hi, vals[x].lo);
  }
  std::vector<size_t> idx(vals.size());
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return top_k_compare(recs.data() + a * stride, recs.data() + b * stride, len) < 0; });
  return idx;
}
static void show_order(const char* name, const TopKKey& k, const std::vector<Val>& vals, int kind) {
  printf("%s", name);
  for (size_t x : order_of(k, vals, kind)) printf(" %zu", x);
  printf("\n");
}
static TopKKey one_key(uint32_t kind, uint32_t desc, uint32_t nf) { return {0, kind, desc, nf, 0, kind == TK_DEC128 ? 17u : 9u}; }
static Val fv(double f) { return {true, f, 0, 0, 0}; }
static Val iv(int64_t i) { return {true, 0, i, 0, 0}; }
static Val dv(__int128 v) { return {true, 0, 0, (uint64_t)((unsigned __int128)v >> 64), (uint64_t)(unsigned __int128)v}; }
static const Val kNull = {false, 0, 0, 0, 0};

static void show_merge(const char* name, const std::vector<std::vector<int64_t>>& stripes, uint32_t k, uint64_t cap) {
  const TopKKey key = one_key(TK_INT, 0, 0);
  std::vector<TopKStripe> in;
  for (auto& s : stripes) {
    TopKStripe t;
    t.n = s.size();
    t.recs.assign(s.size() * top_k_stride(9), 0);
    for (size_t x = 0; x < s.size(); x++) top_k_put_i64(t.recs.data() + x * top_k_stride(9), key, true, s[x]);
    in.push_back(t);
  }
  std::vector<uint64_t> pos(cap + 1, 777);
  uint64_t n = 999;
  const int rc = top_k_merge(in, 9, k, cap ? pos.data() : nullptr, cap, &n);
  printf("%s %d %llu", name, rc, (unsigned long long)n);
  for (uint64_t x = 0; x < cap && x < n && !rc; x++) printf(" %llu", (unsigned long long)pos[x]);
  printf(" guard=%llu\n", (unsigned long long)pos[cap]);
}

int main() {
  // ---- the plan: kinds, flags, where each key's bytes stand ----
  show_plan("one_i64", {key("i64")});
  show_plan("desc_nf", {key("f32", 1, 1)});
  show_plan("four_mixed", {key("dec", 1), key("b"), key("ts_ns", 0, 1), key("i8", 7, 9)});
  show_plan("date", {key("date")});
  show_plan("one_dec", {key("dec")});
  show_passes("i64_dec", {key("i64"), key("dec")});
  show_passes("b", {key("b")});
  // ---- the refusals ----
  show_plan("no_key", {});
  show_plan("five_keys", {key("i64"), key("f32"), key("b"), key("dec"), key("date")});
  show_plan("k_zero", {key("i64")}, 0);
  show_plan("k_max", {key("i64")}, ORCGPU_TOP_K_MAX);
  show_plan("k_over", {key("i64")}, ORCGPU_TOP_K_MAX + 1);
  show_plan("unknown", {key("nope")});
  show_plan("twice", {key("i64"), key("f32"), key("i64", 1)});
  show_plan("string_key", {key("s")});
  show_plan("binary_key", {key("bin")});
  show_plan("dict_key", {key("dict")});
  show_plan("ts_dec_key", {key("ts_dec")});
  show_plan("null_name", {key(nullptr)});
  {
    AggCol cols[2] = {col(ORCGPU_T_LONG, 8), col(ORCGPU_T_STRUCT, 0, false, 3, true)};
    const char* const names[2] = {"i64", "st"};
    const orcgpu_sort_key k1 = key("i64");
    TopKPlan plan;
    const int rc = top_k_compile(&k1, 1, 5, names, cols, 2, plan);
    printf("nested %d\t%s\n", rc, plan.err);
  }
  // ---- the workspace ----
  show_workspace("ws_small", 1000, 9, 10, 70001);
  show_workspace("ws_k_above_rows", 4096, 68, 65536, 63);
  show_workspace("ws_big", 123456789, 26, 65536, 6000000);
  show_workspace("ws_one_row", 256, 9, 1, 1);
  // ---- key records: the hand cases ----
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const std::vector<Val> floats = {fv(nan), fv(inf), fv(-inf), fv(1.5), fv(-nan), fv(0.0)};
  show_order("nan_inf_asc", one_key(TK_FLOAT, 0, 0), floats, TK_FLOAT);
  show_order("nan_inf_desc", one_key(TK_FLOAT, 1, 0), floats, TK_FLOAT);
  const std::vector<Val> zeros = {fv(0.0), fv(-0.0), fv(-0.0), fv(0.0), fv(-1.0)};
  show_order("zeros_asc", one_key(TK_FLOAT, 0, 0), zeros, TK_FLOAT);
  show_order("zeros_desc", one_key(TK_FLOAT, 1, 0), zeros, TK_FLOAT);
  const std::vector<Val> nulls = {iv(3), kNull, iv(1), kNull, iv(2)};
  show_order("nulls_asc", one_key(TK_INT, 0, 0), nulls, TK_INT);
  show_order("nulls_desc", one_key(TK_INT, 1, 0), nulls, TK_INT);
  show_order("nulls_desc_first", one_key(TK_INT, 1, 1), nulls, TK_INT);
  show_order("nulls_asc_first", one_key(TK_INT, 0, 1), nulls, TK_INT);
  const std::vector<Val> ints = {iv(0), iv(INT64_MAX), iv(INT64_MIN), iv(-1), iv(1)};
  show_order("int64_asc", one_key(TK_INT, 0, 0), ints, TK_INT);
  show_order("int64_desc", one_key(TK_INT, 1, 0), ints, TK_INT);
  __int128 big = 1;
  for (int x = 0; x < 37; x++) big *= 10;
  const std::vector<Val> decs = {dv(big), dv(-big), dv(0), dv(-1), kNull};
  show_order("dec_asc", one_key(TK_DEC128, 0, 0), decs, TK_DEC128);
  show_order("dec_desc_first", one_key(TK_DEC128, 1, 1), decs, TK_DEC128);
  const std::vector<Val> bools = {iv(1), iv(0), kNull, iv(1), iv(0)};
  show_order("bools", one_key(TK_BOOL, 0, 0), bools, TK_BOOL);
  {  // four keys where only the last differs: a asc, b desc, c asc nulls first, d asc -- then d desc nulls first
    for (int variant = 0; variant < 2; variant++) {
      TopKKeys keys{};
      keys.n = 4;
      const uint32_t kinds[4] = {TK_INT, TK_FLOAT, TK_BOOL, TK_INT};
      const uint32_t desc[4] = {0, 1, 0, variant ? 1u : 0u}, nf[4] = {0, 0, 1, variant ? 1u : 0u};
      for (uint32_t q = 0; q < 4; q++) keys.key[q] = {q, kinds[q], desc[q], nf[q], q * 9, 9};
      keys.len = 36;
      const uint32_t stride = top_k_stride(36);
      const std::vector<Val> d = {iv(5), iv(3), kNull, iv(4), iv(3)};
      std::vector<uint8_t> recs(d.size() * stride, 0);
      for (size_t x = 0; x < d.size(); x++) {
        uint8_t* r = recs.data() + x * stride;
        top_k_put_i64(r, keys.key[0], true, 1);
        top_k_put_f64(r, keys.key[1], true, 2.5);
        top_k_put_bool(r, keys.key[2], true, true);
        top_k_put_i64(r, keys.key[3], d[x].valid, d[x].i);
      }
      std::vector<size_t> idx(d.size());
      std::iota(idx.begin(), idx.end(), 0);
      std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return top_k_compare(recs.data() + a * stride, recs.data() + b * stride, 36) < 0; });
      printf("four_keys_%d", variant);
      for (size_t x : idx) printf(" %zu", x);
      printf("\n");
    }
  }
  printf("stride %u %u %u %u\n", top_k_stride(9), top_k_stride(17), top_k_stride(26), top_k_stride(68));
  // ---- the merge: 3 stripes, ties across stripes, a stripe with no rows, cap too small ----
  const std::vector<std::vector<int64_t>> three = {{1, 3, 3, 7}, {}, {0, 3, 8}, {3, 3}};
  show_merge("merge_all", three, 100, 16);      // positions: stripe bases 0, 4, 4, 7
  show_merge("merge_k5", three, 5, 5);
  show_merge("merge_cap_small", three, 5, 4);
  show_merge("merge_cap_zero", three, 5, 0);
  show_merge("merge_empty", {{}, {}}, 5, 0);
  show_merge("merge_none", {}, 5, 3);
  return 0;
}
