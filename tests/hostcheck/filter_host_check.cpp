// filter_host_check.cpp -- the row filter call's host arithmetic (orc_rust_amd/csrc/orcgpu_filter_host.inc, the very text
// liborcgpu.so is built from) under AddressSanitizer + UBSan, on the CPU (TEST INFRASTRUCTURE).  filter_col_kind,
// filter_check_kinds, FilterWorkspace and filter_place_output are compared, field by field, with transcriptions of the code blocks
// result_filter_plan held before the arithmetic had functions of its own.  One thing differs from those blocks on purpose: the
// workspace holds one more slot, the leaf lists of the two plane kernels, behind the literal pool; the transcription takes it there.
// A seeded sweep of small shapes, then the offset overflow by hand.
// Prints one line per case; exit code 0 when every case agreed; a sanitizer report aborts with its own exit code.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "../../include/orcgpu.h"
#include "../../orc_rust_amd/csrc/orcgpu_filter_host.inc"

using orcgpu_host::FilterPlan;

// ---- what orcgpu.hip and the device headers held ----
constexpr uint64_t kAlign = 256;
static inline uint64_t align_up(uint64_t v, uint64_t a = kAlign) { return (v + a - 1) / a * a; }
struct Bump {
  uint64_t off = 0;
  uint64_t take(uint64_t n, uint64_t a = kAlign) {
    off = align_up(off, a);
    uint64_t r = off;
    off += n;
    return r;
  }
};
struct RefFilterCol {  // FilterCol
  const unsigned long long* validity;
  const uint8_t* values;
  const int32_t* offsets;
  const unsigned long long* char_base;
  const uint8_t* chars;
  uint32_t width, kind;
};
struct RefGatherJob {  // FilterGatherJob
  RefFilterCol src;
  unsigned long long* out_validity;
  uint8_t* out_values;
  int32_t* out_offsets;
  uint8_t* out_chars;
  const unsigned long long* out_char_base;
};
struct RefSelBatch {
  uint64_t start;
  uint32_t len, pad;
};

static int g_bad = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      g_bad++;                                                             \
      printf("  MISMATCH line %d: %s\n", __LINE__, #cond);                 \
    }                                                                      \
  } while (0)

// ---- the references ----
static uint32_t reference_kind(const FilterColDesc& co) {
  uint32_t kind;
  if (co.is_bool) {
    kind = FKIND_BOOL;
  } else if (co.is_string) {
    kind = FKIND_STRING;
  } else {
    const int ot = co.orc_type;
    const bool is_int = ot == ORCGPU_T_BYTE || ot == ORCGPU_T_SHORT || ot == ORCGPU_T_INT || ot == ORCGPU_T_LONG || ot == ORCGPU_T_DATE;
    const bool is_float = ot == ORCGPU_T_FLOAT || ot == ORCGPU_T_DOUBLE;
    const bool is_ts = (ot == ORCGPU_T_TIMESTAMP || ot == ORCGPU_T_TIMESTAMP_INSTANT) && co.ts_unit <= 3 && co.width == 8;
    const bool is_dec = ot == ORCGPU_T_DECIMAL && co.width == 16;
    kind = (is_int && co.width <= 8) || is_ts ? FKIND_INT
           : (is_float && (co.width == 4 || co.width == 8) ? FKIND_FLOAT : (is_dec ? FKIND_DEC128 : FKIND_OTHER));
  }
  return kind;
}
static int reference_check(const FilterPlan& plan, const std::vector<uint32_t>& kinds, const std::vector<FilterColDesc>& cols, uint32_t* col) {
  const uint32_t nc = (uint32_t)cols.size();
  for (auto& in : plan.prog) {
    if (!fop_reads_values(in.op)) continue;
    *col = in.col;
    if (in.col < nc && cols[in.col].dict_out) return ORCGPU_UNSUPPORTED;
    const uint32_t want = in.op == FOP_IN ? (uint32_t)in.lo : in.op == FOP_CMP_INT ? FKIND_INT : in.op == FOP_CMP_FLOAT ? FKIND_FLOAT : in.op == FOP_CMP_BOOL ? FKIND_BOOL : in.op == FOP_CMP_DEC128 ? FKIND_DEC128 : FKIND_STRING;
    if (in.col >= nc || kinds[in.col] != want) return ORCGPU_MISMATCHED_SCHEMA;
  }
  return ORCGPU_OK;
}
struct Slot {
  const char* name;
  uint64_t off, size;
};
struct RefWorkspace {
  std::vector<Slot> slots;  // in the order they were taken
  uint64_t up_bytes, n_counters, up2_first, up2_bytes, bytes;
};
static RefWorkspace reference_workspace(const FilterPlan& plan, const std::vector<FilterColDesc>& cols, uint32_t n_segs, uint32_t src_batches, uint64_t n_in, uint32_t B) {
  RefWorkspace R;
  const uint32_t nc = (uint32_t)cols.size();
  const uint64_t n_words = (n_in + 63) / 64, nb_max = (n_in + B - 1) / B;
  Bump t;
  auto take = [&](const char* name, uint64_t n) {
    R.slots.push_back({name, t.take(n), n});
    return R.slots.back().off;
  };
  take("prog", plan.prog.size() * sizeof(FilterInsn) + 16);
  take("lits", plan.lits.size() + 16);
  take("leaves", (plan.like_leaves.size() + plan.in_leaves.size()) * 4 + 16);  // (the new slot)
  take("cols", (uint64_t)nc * sizeof(RefFilterCol) + 16);
  take("segs", (uint64_t)n_segs * sizeof(RefSelBatch) + 16);
  take("first", (uint64_t)n_segs * 8 + 16);
  for (uint32_t c = 0; c < nc; c++)
    if (cols[c].is_string) take("cbase", (uint64_t)src_batches * 8 + 16);
  R.up_bytes = t.off;
  take("keep", n_words * 8 + 16);
  take("cnt", n_words * 4 + 16);
  take("woff", n_words * 8 + 16);
  take("sums", ((n_words + 2047) / 2048) * 8 + 16);
  R.n_counters = 1 + 2ull * nc * nb_max;
  take("counters", R.n_counters * 8 + 16);
  take("rows", n_in * 4 + 16);
  const uint64_t n_planes = plan.like_leaves.size() + plan.in_leaves.size();
  take("planes", n_planes * n_words * 8 + 16);
  const uint64_t o_jobs = take("jobs", (uint64_t)nc * sizeof(RefGatherJob) + 16), o_obase = take("obase", (uint64_t)nc * nb_max * 8 + 16);
  R.up2_first = o_jobs;
  R.up2_bytes = o_obase + (uint64_t)nc * nb_max * 8 - o_jobs;
  R.bytes = t.off;
  return R;
}
struct RefPlace {
  uint64_t validity = 0, values = 0, offsets = 0, dict_offsets = 0, dict_values = 0;
  bool has_validity = false;
};
struct RefOutput {
  std::vector<RefPlace> place;
  std::vector<uint64_t> obase;
  uint64_t arena = 0, arrow_bytes = 0;
  uint32_t nbo = 0;
  int status = 0;
  uint32_t err_batch = 0, err_col = 0;
  std::vector<FilterColDesc> cols;  // as the block left them: dict_len / dict_bytes / dict_decoded
  std::vector<std::vector<uint64_t>> null_counts, char_base, char_total;
  std::vector<uint64_t> dict_offsets_off, dict_values_off;
};
static RefOutput reference_output(const std::vector<FilterColDesc>& cols_in, const std::vector<uint64_t>& back, uint64_t nb_max, uint64_t kept, uint32_t B, uint32_t W) {
  RefOutput R;
  R.cols = cols_in;
  const uint32_t nc = (uint32_t)cols_in.size();
  const uint32_t nbo = (uint32_t)((kept + B - 1) / B);
  auto nulls_of = [&](uint32_t c, uint32_t k) { return back[1 + (uint64_t)c * nb_max + k]; };
  auto bytes_of = [&](uint32_t c, uint32_t k) { return back[1 + ((uint64_t)nc + c) * nb_max + k]; };
  Bump a;
  std::vector<uint64_t> obase((size_t)nc * nb_max, 0);
  std::vector<RefPlace> place(nc);
  int status = 0;
  uint32_t err_batch = 0, err_col = 0;
  for (uint32_t c = 0; c < nc; c++) {
    const FilterColDesc& co = R.cols[c];
    RefPlace& p = place[c];
    uint64_t nulls = 0, bytes = 0;
    for (uint32_t k = 0; k < nbo; k++) {
      nulls += nulls_of(c, k);
      obase[(size_t)c * nb_max + k] = bytes;
      bytes += bytes_of(c, k);
      if (co.is_string && bytes_of(c, k) > 0x7fffffffull && (!status || k < err_batch)) {
        status = ORCGPU_OFFSET_OVERFLOW;
        err_batch = k;
        err_col = c;
      }
    }
    p.has_validity = nulls != 0;
    if (p.has_validity) p.validity = a.take((uint64_t)nbo * W * 8 + 16);
    if (co.is_bool) p.values = a.take((uint64_t)nbo * W * 8 + 16);
    else if (co.is_string) {
      p.offsets = a.take((uint64_t)nbo * (B + 1) * 4 + 16);
      p.values = a.take(bytes + 16);
    } else p.values = a.take(kept * co.width + 16);
    if (co.dict_out && co.dict_decoded) {
      p.dict_offsets = a.take((co.dict_len + 1) * 4 + 16);
      p.dict_values = a.take(co.dict_bytes + 16);
    }
  }
  R.arena = a.off;
  R.null_counts.resize(nc);
  R.char_base.resize(nc);
  R.char_total.resize(nc);
  R.dict_offsets_off.assign(nc, 0);
  R.dict_values_off.assign(nc, 0);
  for (uint32_t c = 0; c < nc; c++) {
    FilterColDesc& co = R.cols[c];
    const RefPlace& p = place[c];
    if (co.dict_out) {
      if (!kept) {
        co.dict_len = co.dict_bytes = 0;
        co.dict_decoded = false;
      }
      R.dict_offsets_off[c] = kept ? p.dict_offsets : 0;
      R.dict_values_off[c] = kept ? p.dict_values : 0;
      if (co.dict_decoded) R.arrow_bytes += (co.dict_len + 1) * 4 + co.dict_bytes;
    }
    R.null_counts[c].assign(nbo, 0);
    R.char_base[c].assign(co.is_string ? nbo : 0, 0);
    R.char_total[c].assign(co.is_string ? nbo : 0, 0);
    for (uint32_t k = 0; k < nbo; k++) {
      const uint64_t rows = std::min<uint64_t>(B, kept - (uint64_t)k * B);
      R.null_counts[c][k] = nulls_of(c, k);
      if (co.is_string) {
        R.char_base[c][k] = obase[(size_t)c * nb_max + k];
        R.char_total[c][k] = bytes_of(c, k);
      }
      R.arrow_bytes += co.is_string ? R.char_total[c][k] + 4 * (rows + 1) : (co.is_bool ? (rows + 7) / 8 : rows * co.width);
      if (R.null_counts[c][k]) R.arrow_bytes += (rows + 7) / 8;
    }
  }
  R.place = place;
  R.obase = obase;
  R.nbo = nbo;
  R.status = status;
  R.err_batch = err_batch;
  R.err_col = err_col;
  return R;
}

// ---- the comparisons ----
static void compare_workspace(const FilterPlan& plan, const std::vector<FilterColDesc>& cols, uint32_t n_segs, uint32_t src_batches, uint64_t n_in, uint32_t B) {
  const RefWorkspace R = reference_workspace(plan, cols, n_segs, src_batches, n_in, B);
  const FilterWorkspace ws(plan, cols.data(), (uint32_t)cols.size(), n_segs, src_batches, n_in, B);
  std::vector<uint64_t> got = {ws.o_prog, ws.o_lits, ws.o_leaves, ws.o_cols, ws.o_segs, ws.o_first};
  for (size_t c = 0; c < cols.size(); c++) {
    if (cols[c].is_string) got.push_back(ws.o_cbase[c]);
    else CHECK(ws.o_cbase[c] == 0);
  }
  for (uint64_t o : {ws.o_keep, ws.o_cnt, ws.o_woff, ws.o_sums, ws.o_counters, ws.o_rows, ws.o_planes, ws.o_jobs, ws.o_obase}) got.push_back(o);
  CHECK(got.size() == R.slots.size());
  uint64_t end = 0;
  for (size_t k = 0; k < R.slots.size() && k < got.size(); k++) {
    CHECK(got[k] == R.slots[k].off);
    CHECK(got[k] % 256 == 0 && got[k] >= end);  // 256-byte aligned, behind the slot before
    end = got[k] + R.slots[k].size;
  }
  CHECK(end <= ws.bytes && ws.bytes == R.bytes);
  CHECK(ws.up_bytes == R.up_bytes && ws.up_bytes <= ws.o_keep && ws.n_counters == R.n_counters);
  CHECK(ws.o_jobs == R.up2_first && ws.up2_bytes == R.up2_bytes && ws.o_jobs + ws.up2_bytes <= ws.bytes);
  CHECK(ws.n_words == (n_in + 63) / 64 && ws.nb_max == (n_in + B - 1) / B);
}
static void compare_output(const std::vector<FilterColDesc>& cols, const std::vector<uint64_t>& back, uint64_t nb_max, uint64_t kept, uint32_t B, uint32_t W) {
  const RefOutput R = reference_output(cols, back, nb_max, kept, B, W);
  const FilterOutput out = filter_place_output(cols.data(), back.data(), (uint32_t)cols.size(), nb_max, kept, B, W);
  CHECK(out.nbo == R.nbo && out.arena_bytes == R.arena && out.arrow_bytes == R.arrow_bytes && out.obase == R.obase);
  CHECK(out.status == R.status && out.err_batch == R.err_batch && out.err_col == R.err_col);
  CHECK(out.place.size() == cols.size());
  for (size_t c = 0; c < cols.size() && c < out.place.size(); c++) {
    const FilterPlace& p = out.place[c];
    const RefPlace& q = R.place[c];
    CHECK(p.validity == q.validity && p.values == q.values && p.offsets == q.offsets && p.dict_offsets == q.dict_offsets && p.dict_values == q.dict_values);
    CHECK(p.has_validity == q.has_validity);
    CHECK(p.null_counts == R.null_counts[c] && p.char_base == R.char_base[c] && p.char_total == R.char_total[c]);
    CHECK(p.dict_kept == (cols[c].dict_out && kept != 0));
    CHECK((p.dict_kept ? p.dict_offsets : 0) == R.dict_offsets_off[c] && (p.dict_kept ? p.dict_values : 0) == R.dict_values_off[c]);
    for (uint64_t o : {p.validity, p.values, p.offsets, p.dict_offsets, p.dict_values}) CHECK(o % 256 == 0 && o <= out.arena_bytes);
  }
}

static FilterColDesc random_col(std::mt19937_64& rng) {
  static const int32_t types[] = {ORCGPU_T_BYTE, ORCGPU_T_SHORT, ORCGPU_T_INT, ORCGPU_T_LONG, ORCGPU_T_DATE, ORCGPU_T_FLOAT, ORCGPU_T_DOUBLE, ORCGPU_T_DECIMAL,
                                  ORCGPU_T_TIMESTAMP, ORCGPU_T_TIMESTAMP_INSTANT, ORCGPU_T_BINARY};
  static const uint32_t widths[] = {1, 2, 4, 8, 16};
  FilterColDesc d;
  d.has_present = rng() % 2;
  d.ts_unit = (int32_t)(rng() % 5);
  switch (rng() % 4) {
    case 0:
      d.orc_type = ORCGPU_T_BOOLEAN;
      d.is_bool = true;
      break;
    case 1:
      d.orc_type = ORCGPU_T_STRING;
      d.is_string = true;
      break;
    case 2:  // a string column handed out as dictionary keys: an int32 column with the stripe's dictionary beside it
      d.orc_type = ORCGPU_T_STRING;
      d.width = 4;
      d.dict_out = true;
      d.dict_decoded = rng() % 4 != 0;
      d.dict_len = d.dict_decoded ? rng() % 50 : 0;
      d.dict_bytes = d.dict_decoded ? rng() % 700 : 0;
      break;
    default:
      d.orc_type = types[rng() % (sizeof(types) / sizeof(types[0]))];
      d.width = widths[rng() % 5];
  }
  return d;
}

int main() {
  std::mt19937_64 rng(20260101);
  int cases = 0;
  // ---- every kind rule: each type at each width and unit ----
  for (int32_t ot = 0; ot <= 20; ot++)
    for (uint32_t width : {0u, 1u, 2u, 4u, 8u, 16u})
      for (int32_t unit = 0; unit <= 4; unit++)
        for (int shape = 0; shape < 3; shape++) {
          FilterColDesc d;
          d.orc_type = ot;
          d.width = width;
          d.ts_unit = unit;
          d.is_bool = shape == 1;
          d.is_string = shape == 2;
          CHECK(filter_col_kind(d) == reference_kind(d));
        }
  printf("kinds %d\n", g_bad);
  // ---- the sweep ----
  for (uint32_t B : {1u, 64u, 100u, 8192u}) {
    const uint32_t W = (B + 63) / 64;
    for (uint64_t kept : {(uint64_t)0, (uint64_t)1, (uint64_t)B - 1, (uint64_t)B, (uint64_t)B + 1, (uint64_t)3 * B})
      for (uint32_t nc = 0; nc <= 5; nc++)
        for (uint32_t n_segs : {0u, 1u, 3u})
          for (int with_nulls = 0; with_nulls < 2; with_nulls++) {
            const int before = g_bad;
            std::vector<FilterColDesc> cols;
            for (uint32_t c = 0; c < nc; c++) cols.push_back(random_col(rng));
            const uint64_t n_in = kept + rng() % (2 * B + 1);
            const uint64_t nb_max = (n_in + B - 1) / B;
            FilterPlan plan;
            plan.prog.resize(rng() % 9);
            plan.lits.resize(rng() % 3 ? rng() % 3000 : 0);
            plan.like_leaves.resize(rng() % 3);
            plan.in_leaves.resize(rng() % 3);
            for (auto& in : plan.prog) {  // (columns past the table among them)
              in.op = (uint32_t)(rng() % 15);
              in.col = (uint32_t)(rng() % (nc + 2));
              in.lo = rng() % 6;
            }
            compare_workspace(plan, cols, n_segs, (uint32_t)(rng() % 40), n_in, B);
            std::vector<uint32_t> kinds;
            for (auto& d : cols) kinds.push_back(filter_col_kind(d));
            uint32_t col_a = ~0u, col_b = ~0u;
            const int rc_a = filter_check_kinds(plan, kinds.data(), cols.data(), nc, &col_a), rc_b = reference_check(plan, kinds, cols, &col_b);
            CHECK(rc_a == rc_b && (!rc_a || col_a == col_b));
            // what the one wait fetched: the counts of the batches the kept rows fill, zero behind them
            std::vector<uint64_t> back(1 + 2ull * nc * nb_max, 0);
            back[0] = kept;
            for (uint32_t c = 0; c < nc; c++)
              for (uint64_t k = 0; k * B < kept; k++) {
                const uint64_t rows = std::min<uint64_t>(B, kept - k * B);
                if (with_nulls && cols[c].has_present) back[1 + (uint64_t)c * nb_max + k] = rng() % (rows + 1);
                if (cols[c].is_string) back[1 + ((uint64_t)nc + c) * nb_max + k] = rng() % 3 ? rng() % (40 * rows) : 0;
              }
            compare_output(cols, back, nb_max, kept, B, W);
            cases++;
            if (g_bad != before) printf("case B=%u kept=%llu nc=%u n_segs=%u nulls=%d: MISMATCH\n", B, (unsigned long long)kept, nc, n_segs, with_nulls);
          }
  }
  printf("sweep %d %d\n", cases, g_bad);
  // ---- a batch of 0x80000000 string bytes: ORCGPU_OFFSET_OVERFLOW with the lowest failing batch, whichever column holds it ----
  {
    const uint32_t B = 64, W = 1, nc = 3;
    const uint64_t kept = 3 * B, nb_max = 4;
    std::vector<FilterColDesc> cols(nc);
    cols[0].orc_type = ORCGPU_T_LONG;
    cols[0].width = 8;
    cols[1].orc_type = cols[2].orc_type = ORCGPU_T_STRING;
    cols[1].is_string = cols[2].is_string = true;
    std::vector<uint64_t> back(1 + 2ull * nc * nb_max, 0);
    back[0] = kept;
    auto bytes = [&](uint32_t c, uint32_t k) -> uint64_t& { return back[1 + ((uint64_t)nc + c) * nb_max + k]; };
    bytes(1, 0) = 0x7fffffffull;  // the most a batch may hold
    bytes(1, 2) = 0x80000000ull;
    bytes(2, 1) = 0x80000000ull;  // the lowest failing batch, in the later column
    bytes(2, 2) = 0x80000005ull;
    compare_output(cols, back, nb_max, kept, B, W);
    const FilterOutput out = filter_place_output(cols.data(), back.data(), nc, nb_max, kept, B, W);
    CHECK(out.status == ORCGPU_OFFSET_OVERFLOW && out.err_batch == 1 && out.err_col == 2);
    printf("overflow %d %u %u\n", out.status, out.err_batch, out.err_col);
    bytes(2, 1) = 0x7fffffffull;
    bytes(2, 2) = 5;
    const FilterOutput out2 = filter_place_output(cols.data(), back.data(), nc, nb_max, kept, B, W);
    CHECK(out2.status == ORCGPU_OFFSET_OVERFLOW && out2.err_batch == 2 && out2.err_col == 1);
    printf("overflow %d %u %u\n", out2.status, out2.err_batch, out2.err_col);
    bytes(1, 2) = 0x7fffffffull;
    const FilterOutput out3 = filter_place_output(cols.data(), back.data(), nc, nb_max, kept, B, W);
    CHECK(out3.status == 0);
    printf("overflow %d %u %u\n", out3.status, out3.err_batch, out3.err_col);
  }
  static_assert(sizeof(RefFilterCol) == kFilterColBytes && sizeof(RefGatherJob) == kFilterJobBytes && sizeof(RefSelBatch) == kFilterSegBytes && kAlign == kFilterAlign, "");
  printf("bad %d\n", g_bad);
  return g_bad ? 1 : 0;
}
