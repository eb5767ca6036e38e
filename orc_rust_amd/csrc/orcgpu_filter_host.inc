// orcgpu_filter_host.inc -- what a row filter call works out on the host with plain arithmetic: what kind a decoded column is to
// the kernels (filter_col_kind), whether the plan fits the decoded columns (filter_check_kinds), where everything lies in the
// filter's workspace (FilterWorkspace) and, behind the one wait, where the kept rows go (filter_place_output).
//
// No HIP in this file and nothing of the context or the result: tests/hostcheck/filter_host_check.cpp compiles it for the host,
// under AddressSanitizer, against transcriptions of the code blocks result_filter_plan held before.  The alignment and the sizes
// of the three device structs it lays out are stated here; orcgpu_filter.inc ties them to the originals with a static_assert.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "orcgpu_filter_plan.inc"

namespace {

constexpr uint64_t kFilterAlign = 256;    // kAlign (orcgpu.hip)
constexpr uint64_t kFilterColBytes = 48;  // sizeof(FilterCol), sizeof(FilterGatherJob) (device/filter_kernels.hip), sizeof(SelBatch)
constexpr uint64_t kFilterJobBytes = 88;
constexpr uint64_t kFilterSegBytes = 16;

struct FilterBump {  // Bump (orcgpu.hip)
  uint64_t off = 0;
  uint64_t take(uint64_t n) {
    off = (off + kFilterAlign - 1) / kFilterAlign * kFilterAlign;
    const uint64_t r = off;
    off += n;
    return r;
  }
};

// What the filter reads of a decoded column (ColumnOut)
struct FilterColDesc {
  int32_t orc_type = 0;
  uint32_t width = 0;
  int32_t ts_unit = 3;
  bool is_bool = false, is_string = false, has_present = false;
  bool dict_out = false, dict_decoded = false;
  uint64_t dict_len = 0, dict_bytes = 0;
};

// FKIND_*: what the kernels may do with the column's values
inline uint32_t filter_col_kind(const FilterColDesc& d) {
  if (d.is_bool) return FKIND_BOOL;
  if (d.is_string) return FKIND_STRING;
  const int ot = d.orc_type;
  const bool is_int = ot == ORCGPU_T_BYTE || ot == ORCGPU_T_SHORT || ot == ORCGPU_T_INT || ot == ORCGPU_T_LONG || ot == ORCGPU_T_DATE;
  const bool is_float = ot == ORCGPU_T_FLOAT || ot == ORCGPU_T_DOUBLE;
  // (a value narrower or wider than the type's own -- with_schema -- is still compared as what it is: 1 / 2 / 4 / 8 bytes)
  // (a Timestamp decoded to an int64 unit is compared as the integer it is; decoded to Decimal128(38, 9) it is not compared)
  const bool is_ts = (ot == ORCGPU_T_TIMESTAMP || ot == ORCGPU_T_TIMESTAMP_INSTANT) && d.ts_unit <= 3 && d.width == 8;
  const bool is_dec = ot == ORCGPU_T_DECIMAL && d.width == 16;
  return (is_int && d.width <= 8) || is_ts ? FKIND_INT : (is_float && (d.width == 4 || d.width == 8) ? FKIND_FLOAT : (is_dec ? FKIND_DEC128 : FKIND_OTHER));
}

// The one text of the dictionary-column refusal, for whoever finds it: the call's check against a decoded result (filter_check,
// orcgpu_filter.inc) and the plan compiler of the aggregates' conditions (agg_compile_conds, orcgpu_agg_plan.inc).  name: the
// column's, or null where only its id is known.
inline void filter_dict_refusal(char* out, size_t n, const char* name, uint32_t column_id) {
  if (name) snprintf(out, n, "row filter: column '%s' is read as a dictionary column: a comparison on its keys is not supported", name);
  else snprintf(out, n, "row filter: column %u is read as a dictionary column: a comparison on its keys is not supported", column_id);
}

// The plan was compiled against the columns' types; what the decode made of them must fit.  ORCGPU_OK, or for the first
// instruction that does not fit: ORCGPU_UNSUPPORTED (it reads the values of a dictionary-output column: string predicates evaluated
// on the entries are not there yet) or ORCGPU_MISMATCHED_SCHEMA (no such column, or not decoded to the kind it compares), with
// the instruction's column in *col.
inline int filter_check_kinds(const orcgpu_host::FilterPlan& plan, const uint32_t* kinds, const FilterColDesc* descs, uint32_t nc, uint32_t* col) {
  for (auto& in : plan.prog) {
    if (in.op == FOP_CMP_EXPR) {  // every column either side names: there, and -- where its values are read -- decoded to what the op loads
      std::vector<orcgpu_host::FilterExprRead> reads;
      orcgpu_host::filter_expr_reads(plan, in, reads);
      if (reads.empty()) return ORCGPU_MISMATCHED_SCHEMA;  // (a leaf without its op tables)
      for (const auto& rd : reads) {
        *col = rd.col;
        if (rd.col >= nc) return ORCGPU_MISMATCHED_SCHEMA;
        if (rd.kind == orcgpu_host::kFilterExprAnyKind) continue;
        if (descs[rd.col].dict_out) return ORCGPU_UNSUPPORTED;
        if (kinds[rd.col] != rd.kind) return ORCGPU_MISMATCHED_SCHEMA;
      }
      continue;
    }
    if (!fop_reads_values(in.op)) continue;
    *col = in.col;
    if (in.col < nc && descs[in.col].dict_out) return ORCGPU_UNSUPPORTED;
    if (in.col >= nc || kinds[in.col] != fop_value_kind(in.op, in.lo)) return ORCGPU_MISMATCHED_SCHEMA;
  }
  return ORCGPU_OK;
}

// The filter's temporaries, one allocation that only ever grows: the tables that go up in one copy [0, up_bytes), what the kernels
// leave, and the second upload behind the wait [o_jobs, o_jobs + up2_bytes): the gather's jobs and the output batches' char bases.
struct FilterWorkspace {
  uint64_t n_words = 0, nb_max = 0;  // 64-bit words of a mask over the input rows; output batches at most
  uint64_t o_prog = 0, o_lits = 0, o_leaves = 0, o_cols = 0, o_segs = 0, o_first = 0, up_bytes = 0;  // (o_leaves: the LIKE leaves, the IN leaves, the expression leaves)
  std::vector<uint64_t> o_cbase;  // per string column: the char bases of the decode's uniform batches
  uint64_t o_keep = 0, o_cnt = 0, o_woff = 0, o_sums = 0, o_counters = 0, o_rows = 0, o_planes = 0;
  uint64_t n_counters = 0;  // the kept row count, then null counts and string bytes [column][batch]
  // ... and ONE word behind them (in the 16 bytes every part is given beyond its size), zeroed and fetched with them: the (row, leaf)
  // evaluations of the expression leaves in which an operation left 128 bits (filter_expr_kernel)
  uint64_t o_overflow = 0;
  uint64_t o_jobs = 0, o_obase = 0, up2_bytes = 0;
  uint64_t bytes = 0;

  // (out_rows_max: a caller that hands out fewer rows than it takes in -- the top-k -- sizes the output batches by them)
  FilterWorkspace(const orcgpu_host::FilterPlan& plan, const FilterColDesc* descs, uint32_t nc, uint32_t n_segs, uint32_t src_batches, uint64_t n_in, uint32_t B,
                  uint64_t out_rows_max = ~0ull) {
    FilterBump t;
    n_words = (n_in + 63) / 64;
    nb_max = (std::min(n_in, out_rows_max) + B - 1) / B;
    o_prog = t.take(plan.prog.size() * sizeof(FilterInsn) + 16);
    o_lits = t.take(plan.lits.size() + 16);
    o_leaves = t.take(plan.n_planes() * 4 + 16);  // (an expression leaf has two planes and one entry)
    o_cols = t.take((uint64_t)nc * kFilterColBytes + 16);
    o_segs = t.take((uint64_t)n_segs * kFilterSegBytes + 16);
    o_first = t.take((uint64_t)n_segs * 8 + 16);
    o_cbase.assign(nc, 0);
    for (uint32_t c = 0; c < nc; c++)
      if (descs[c].is_string) o_cbase[c] = t.take((uint64_t)src_batches * 8 + 16);
    up_bytes = t.off;
    o_keep = t.take(n_words * 8 + 16);
    o_cnt = t.take(n_words * 4 + 16);
    o_woff = t.take(n_words * 8 + 16);
    o_sums = t.take(((n_words + 2047) / 2048) * 8 + 16);
    n_counters = 1 + 2ull * nc * nb_max;
    o_counters = t.take(n_counters * 8 + 16);
    o_overflow = o_counters + n_counters * 8;
    o_rows = t.take(n_in * 4 + 16);
    // (the LIKE and IN leaves' planes of match bits, numbered together and laid out like `keep`)
    o_planes = t.take((uint64_t)plan.n_planes() * n_words * 8 + 16);
    o_jobs = t.take((uint64_t)nc * kFilterJobBytes + 16);
    o_obase = t.take((uint64_t)nc * nb_max * 8 + 16);
    up2_bytes = o_obase + (uint64_t)nc * nb_max * 8 - o_jobs;
    bytes = t.off;
  }
};

// Where a column of the kept rows lies in the output arena, and what the host knows of its batches
struct FilterPlace {
  uint64_t validity = 0, values = 0, offsets = 0, dict_offsets = 0, dict_values = 0;
  bool has_validity = false;
  bool dict_kept = false;  // a dictionary-output column with rows left to refer to its dictionary
  std::vector<uint64_t> null_counts, char_base, char_total;  // per output batch (the latter two: strings)
};
struct FilterOutput {
  std::vector<FilterPlace> place;
  std::vector<uint64_t> obase;  // [column][nb_max]: what goes up as the output batches' char bases
  uint32_t nbo = 0;             // output batches
  uint64_t arena_bytes = 0;
  uint64_t arrow_bytes = 0;
  int status = 0;               // ORCGPU_OFFSET_OVERFLOW: a batch of a string column holds more than 2^31 - 1 bytes ...
  uint32_t err_batch = 0, err_col = 0;  // ... the lowest such batch, and its column
};

// The output arena, compact: per column what a decode of `kept` rows would hold.  counters: what the one wait fetched
// (FilterWorkspace::n_counters of them).
inline FilterOutput filter_place_output(const FilterColDesc* descs, const uint64_t* counters, uint32_t nc, uint64_t nb_max, uint64_t kept, uint32_t B, uint32_t W) {
  FilterOutput out;
  const uint32_t nbo = out.nbo = (uint32_t)((kept + B - 1) / B);
  auto nulls_of = [&](uint32_t c, uint32_t k) { return counters[1 + (uint64_t)c * nb_max + k]; };
  auto bytes_of = [&](uint32_t c, uint32_t k) { return counters[1 + ((uint64_t)nc + c) * nb_max + k]; };
  FilterBump a;
  out.place.resize(nc);
  out.obase.assign((size_t)nc * nb_max, 0);
  for (uint32_t c = 0; c < nc; c++) {
    const FilterColDesc& co = descs[c];
    FilterPlace& p = out.place[c];
    p.null_counts.assign(nbo, 0);
    p.char_base.assign(co.is_string ? nbo : 0, 0);
    p.char_total.assign(co.is_string ? nbo : 0, 0);
    uint64_t nulls = 0, bytes = 0;
    for (uint32_t k = 0; k < nbo; k++) {
      const uint64_t rows = std::min<uint64_t>(B, kept - (uint64_t)k * B);
      nulls += p.null_counts[k] = nulls_of(c, k);
      out.obase[(size_t)c * nb_max + k] = bytes;
      bytes += bytes_of(c, k);
      if (co.is_string) {
        p.char_base[k] = out.obase[(size_t)c * nb_max + k];
        p.char_total[k] = bytes_of(c, k);
        // OffsetOverflow (string.rs:139-140: the offsets of a batch are i32), as the decoder's check of its uniform batches
        if (bytes_of(c, k) > 0x7fffffffull && (!out.status || k < out.err_batch)) {
          out.status = ORCGPU_OFFSET_OVERFLOW;
          out.err_batch = k;
          out.err_col = c;
        }
      }
      out.arrow_bytes += co.is_string ? p.char_total[k] + 4 * (rows + 1) : (co.is_bool ? (rows + 7) / 8 : rows * co.width);
      if (p.null_counts[k]) out.arrow_bytes += (rows + 7) / 8;
    }
    p.has_validity = nulls != 0;
    if (p.has_validity) p.validity = a.take((uint64_t)nbo * W * 8 + 16);
    if (co.is_bool) p.values = a.take((uint64_t)nbo * W * 8 + 16);
    else if (co.is_string) {
      p.offsets = a.take((uint64_t)nbo * (B + 1) * 4 + 16);
      p.values = a.take(bytes + 16);
    } else p.values = a.take(kept * co.width + 16);
    p.dict_kept = co.dict_out && kept;
    if (co.dict_out && co.dict_decoded) {  // the stripe's dictionary goes along untouched: this arena is all that is copied back
      p.dict_offsets = a.take((co.dict_len + 1) * 4 + 16);
      p.dict_values = a.take(co.dict_bytes + 16);
      if (p.dict_kept) out.arrow_bytes += (co.dict_len + 1) * 4 + co.dict_bytes;
    }
  }
  out.arena_bytes = a.off;
  return out;
}

}  // namespace
