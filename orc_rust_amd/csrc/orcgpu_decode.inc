// orcgpu_decode.inc -- planning + launch sequence of orcgpu_decode_staged (included by orcgpu.hip).

namespace {

// A lane's host clock (us) at the ends of the parts of a decode call (orcgpu_last_lane_host_us, the ORCGPU_DEBUG report)
struct LaneClock {
  double t0 = 0, cols = 0, dp = 0, plan = 0, launch = 0, first = 0, walk = 0, pres = 0, exp = 0, fin = 0, dict = 0, enq = 0, sync = 0;
};

// The tables of compute_columns_kernel as one upload (orcgpu_computed.inc): the columns, the jobs, the programs, the selection's batches
struct ComputedTable {
  uint64_t o_cols = 0, o_jobs = 0, o_ops = 0, o_segs = 0, bytes = 0;
};

// What the steps of decode_lane share: one lane's share of a decode call, from its plan to the pointers its launches take.
struct LaneRun {
  orcgpu_ctx* ctx;
  hipStream_t st;
  orcgpu_staged* const* stripes;
  uint32_t n;
  orcgpu_result** results;
  const std::vector<std::vector<uint8_t>>* mask;  // the lane's columns per stripe (null: all)
  bool host_prof;                                 // ORCGPU_DEBUG
  Plan P;
  DecompPlan DP;
  JobLayout L;
  std::vector<RleHint> hints;  // verified run starts (orcgpu_stream::entries): one table for the call, a slice per job
  // workspace offsets: the per-block arrays (RleBlocks), the hint table, the maps of the exact parallel walk, the summary
  struct {
    uint64_t entry, exit_, nvals, voff, tbase, tsum, flags, badmap, gjob, hint;
  } blk_off{};
  uint64_t hints_off = 0;
  bool use_exact = false;
  uint32_t n_xspans = 0;
  uint64_t x_fmap = 0, x_gmap = 0, x_tile = 0, x_span = 0;
  SummaryLayout SL;
  uint64_t summary_off = 0;
  // the workspace, the summary's host mirror and device copy, and what lies in them
  uint8_t *S = nullptr, *hs = nullptr, *dsum = nullptr;
  RleJob *hjobs = nullptr, *d_jobs = nullptr;
  uint64_t* d_scalars = nullptr;
  unsigned long long *d_nullc = nullptr, *d_chartot = nullptr;
  RleBlocks blk{};
  uint32_t* d_tsum = nullptr;
  int njobs = 0;
  LaneClock ht;
  // computed columns (orcgpu_computed.inc): per stripe that carries them, where their counts lie in the summary and the kernel's
  // tables in the workspace
  struct ComputedPlace {
    uint32_t stripe = 0, first_col = 0, nullcount_off = 0;
    uint64_t table_off = 0;
    ComputedTable tab;
  };
  std::vector<ComputedPlace> computed;
  // lookup columns (orcgpu_lookup.inc): per stripe that carries them, where their counts lie in the summary and the jobs in the workspace
  struct LookupPlace {
    uint32_t stripe = 0, first_col = 0, n_cols = 0, nullcount_off = 0;
    uint64_t table_off = 0;
  };
  std::vector<LookupPlace> lookup;

  uint8_t* arena(const orcgpu_result* r) const { return r->arena[ctx->lane_id].p; }
  // a column's validity words and their ranks (null: no validity)
  const unsigned long long* vbits(const ColPlan& cp) const { return cp.has_present ? reinterpret_cast<const unsigned long long*>(S + cp.vbits_off) : nullptr; }
  const uint32_t* rank(const ColPlan& cp) const { return cp.has_present ? reinterpret_cast<const uint32_t*>(S + cp.rank_off) : nullptr; }
  const uint64_t* h_scalars() const { return reinterpret_cast<const uint64_t*>(hs + SL.scalars_off); }
  const unsigned long long* h_nullc() const { return reinterpret_cast<const unsigned long long*>(hs + SL.nullc_off); }
  const unsigned long long* h_chartot() const { return reinterpret_cast<const unsigned long long*>(hs + SL.chartot_off); }
};

}  // namespace

#include "orcgpu_ext.inc"
#include "orcgpu_lookup.inc"
#include "orcgpu_computed.inc"

namespace {

int ts_unit_of(const orcgpu_column& c) {
  switch (c.arrow_target) {
    case ORCGPU_ARROW_TIMESTAMP_S: case ORCGPU_ARROW_TIMESTAMP_S_UTC: case ORCGPU_ARROW_TIMESTAMP_S_NOTZ: return 0;
    case ORCGPU_ARROW_TIMESTAMP_MS: case ORCGPU_ARROW_TIMESTAMP_MS_UTC: case ORCGPU_ARROW_TIMESTAMP_MS_NOTZ: return 1;
    case ORCGPU_ARROW_TIMESTAMP_US: case ORCGPU_ARROW_TIMESTAMP_US_UTC: case ORCGPU_ARROW_TIMESTAMP_US_NOTZ: return 2;
    case ORCGPU_ARROW_DECIMAL128: return 4;  // Decimal128(38, 9): nanoseconds as i128 (timestamp.rs:96-123)
    default: return 3;  // schema.rs:36-37: nanoseconds by default
  }
}

// array_decoder_factory's match (mod.rs:390-511; timestamps: timestamp.rs:149-232): 0 = this (ORC type, hinted Arrow type) pair
// has a decoder, else the OrcError it raises
int schema_pair_status(const orcgpu_column& c) {
  const int a = c.arrow_target;
  if (a == ORCGPU_ARROW_DEFAULT) return 0;
  const bool unit_default = a >= ORCGPU_ARROW_TIMESTAMP_S && a <= ORCGPU_ARROW_TIMESTAMP_NS;
  switch (c.orc_type) {
    case ORCGPU_T_BOOLEAN: return a == ORCGPU_ARROW_BOOLEAN ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    case ORCGPU_T_BYTE: return a == ORCGPU_ARROW_INT8 ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    case ORCGPU_T_SHORT: return a == ORCGPU_ARROW_INT16 ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    case ORCGPU_T_INT: return a == ORCGPU_ARROW_INT32 ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    case ORCGPU_T_LONG: return a == ORCGPU_ARROW_INT64 ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    case ORCGPU_T_FLOAT: return a == ORCGPU_ARROW_FLOAT32 ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    case ORCGPU_T_DOUBLE: return a == ORCGPU_ARROW_FLOAT64 ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    case ORCGPU_T_STRING: case ORCGPU_T_VARCHAR: case ORCGPU_T_CHAR:
      return a == ORCGPU_ARROW_UTF8 || a == ORCGPU_ARROW_DICTIONARY_UTF8 ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    case ORCGPU_T_BINARY: return a == ORCGPU_ARROW_BINARY ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    case ORCGPU_T_DATE: return a == ORCGPU_ARROW_DATE32 ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    case ORCGPU_T_DECIMAL:
      return (a == ORCGPU_ARROW_DECIMAL128 && (c.precision & 0xff) == c.arrow_precision && (int8_t)c.scale == (int8_t)c.arrow_scale) ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    case ORCGPU_T_TIMESTAMP:
      if (unit_default || (a >= ORCGPU_ARROW_TIMESTAMP_S_NOTZ && a <= ORCGPU_ARROW_TIMESTAMP_NS_NOTZ)) return 0;
      return (a == ORCGPU_ARROW_DECIMAL128 && c.arrow_precision == 38 && c.arrow_scale == 9) ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    case ORCGPU_T_TIMESTAMP_INSTANT:
      if (unit_default || (a >= ORCGPU_ARROW_TIMESTAMP_S_UTC && a <= ORCGPU_ARROW_TIMESTAMP_NS_UTC)) return 0;
      if (a == ORCGPU_ARROW_TIMESTAMP_OTHER_TZ) return ORCGPU_UNSUPPORTED;  // "Non-UTC Arrow timestamps"
      return (a == ORCGPU_ARROW_DECIMAL128 && c.arrow_precision == 38 && c.arrow_scale == 9) ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    // mod.rs:464-505: a nested column takes the nested Arrow type of its kind (its children are checked pair by pair themselves)
    case ORCGPU_T_STRUCT: return a == ORCGPU_ARROW_STRUCT ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    case ORCGPU_T_LIST: return a == ORCGPU_ARROW_LIST ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    case ORCGPU_T_MAP: return a == ORCGPU_ARROW_MAP ? 0 : (a == ORCGPU_ARROW_MAP_SORTED ? ORCGPU_UNSUPPORTED : ORCGPU_MISMATCHED_SCHEMA);
    case ORCGPU_T_UNION: return a == ORCGPU_ARROW_UNION ? 0 : ORCGPU_MISMATCHED_SCHEMA;
    default: return 0;
  }
}

// validity scratch of a column or of a Union's arm: words, their popcounts and ranks
void take_validity_scratch(Plan& P, ColPlan& cp) {
  cp.n_words = (cp.n_rows + 63) / 64;
  cp.n_rank_tiles = (cp.n_words + 1023) / 1024;
  cp.vbits_off = P.scratch.take(cp.n_words * 8 + 16);
  cp.wpop_off = P.scratch.take(cp.n_words * 4);
  cp.rank_off = P.scratch.take(cp.n_words * 4);
  cp.rank_tiles_off = P.scratch.take(cp.n_rank_tiles * 4);
}

// Where the column's DATA job writes: dense in the workspace (`scratch_bytes`; a finisher spaces the values over the rows), or
// straight into the result; either way behind `lead` bytes, the values of the rows before an entry point
void place_dense(Plan& P, ColPlan& cp, ColumnOut& co, uint64_t scratch_bytes, uint64_t lead, bool in_result) {
  JobPlan& j = P.jobs[cp.job_data];
  if (in_result) {
    j.out_result_off = co.values_off;
    j.result_index = cp.stripe;
    co.values_off += lead;
  } else {
    cp.dense_off = P.scratch.take(scratch_bytes);
    j.out_scratch_off = cp.dense_off;
    cp.dense_off += lead;
  }
}

int plan_parent(Plan& P, ColPlan& cp, orcgpu_staged* s);
int plan_present(Plan& P, ColPlan& cp, orcgpu_staged* s, orcgpu_result* r);
int plan_union(Plan& P, ColPlan& cp, orcgpu_staged* s, orcgpu_result* r);
int plan_values(Plan& P, ColPlan& cp, orcgpu_staged* s, orcgpu_result* r);

// Build the plan of one column of one stripe.  Returns an ORCGPU_* status.
int plan_column(Plan& P, int si, int ci, orcgpu_staged* s, orcgpu_result* r) {
  const orcgpu_column& c = s->cols[ci];
  ColPlan cp{};
  cp.stripe = si;
  cp.col = ci;
  cp.c = c;
  cp.n_rows = s->desc.n_rows;
  const uint64_t n = cp.n_rows;
  ColumnOut& co = r->cols[ci];
  co.orc_type = c.orc_type;
  co.column_id = c.column_id;
  co.width = type_width(c.orc_type);
  co.is_string = is_string_type(c.orc_type);
  co.is_bool = c.orc_type == ORCGPU_T_BOOLEAN;
  // int32 keys + the stripe's dictionary instead of Utf8: from here on the column's values are an Int32 column's
  co.dict_out = cp.dict_out = co.is_string && c.arrow_target == ORCGPU_ARROW_DICTIONARY_UTF8;
  co.dict_offsets_off = co.dict_values_off = co.dict_len = co.dict_bytes = 0;
  co.dict_decoded = false;
  if (co.dict_out) {
    co.is_string = false;
    co.width = 4;
  }
  co.precision = c.precision;
  co.scale = c.scale;
  co.ts_unit = ts_unit_of(c);
  co.null_counts.assign(r->n_batches, 0);
  co.status = 0;
  co.lane = s->ctx ? P.lane_id : 0;

  switch (c.orc_type) {
    case ORCGPU_T_BOOLEAN: case ORCGPU_T_BYTE: case ORCGPU_T_SHORT: case ORCGPU_T_INT: case ORCGPU_T_LONG: case ORCGPU_T_FLOAT:
    case ORCGPU_T_DOUBLE: case ORCGPU_T_DATE: case ORCGPU_T_TIMESTAMP: case ORCGPU_T_TIMESTAMP_INSTANT:
    case ORCGPU_T_STRING: case ORCGPU_T_VARCHAR: case ORCGPU_T_CHAR: case ORCGPU_T_BINARY: case ORCGPU_T_DECIMAL:
    case ORCGPU_T_STRUCT: case ORCGPU_T_LIST: case ORCGPU_T_MAP: case ORCGPU_T_UNION:
      break;
    default:
      set_err(s->ctx, "column %u: ORC type kind %d is not decoded on the GPU path", c.column_id, c.orc_type);
      return ORCGPU_UNSUPPORTED;
  }

  if (int ms = schema_pair_status(c)) {
    set_err(s->ctx, ms == ORCGPU_UNSUPPORTED ? (c.orc_type == ORCGPU_T_MAP ? "column %u: Sorted map" : "column %u: Non-UTC Arrow timestamps") : "column %u: mismatched schema: ORC type kind %d cannot be decoded into Arrow type code %d",
            c.column_id, c.orc_type, c.arrow_target);
    return ms;
  }
  cp.err_idx = P.new_scalar(RLE_NO_ERR);
  cp.dicterr_idx = P.new_scalar(RLE_NO_ERR);
  cp.utf8err_idx = P.new_scalar(RLE_NO_ERR);
  cp.nonnull_idx = P.new_scalar(n);
  cp.nullcount_off = (uint32_t)P.n_nullcount_slots;
  P.n_nullcount_slots += r->n_batches;

  // the Struct this column is a field of (orcgpu_column::parent): its validity, if it has any, is merged into this column's
  co.is_struct = c.orc_type == ORCGPU_T_STRUCT;
  co.is_union = c.orc_type == ORCGPU_T_UNION;
  co.parent = c.parent ? (int32_t)c.parent - 1 : -1;
  if (int st = plan_parent(P, cp, s)) return st;
  if (int st = plan_present(P, cp, s, r)) return st;
  if (co.is_struct) {
    cp.ceil8_idx = P.new_scalar((n + 7) / 8);
    P.cols.push_back(cp);
    return ORCGPU_OK;
  }
  return co.is_union ? plan_union(P, cp, s, r) : plan_values(P, cp, s, r);
}

// The Struct, or the arm of a Union, above the column: its depth below it, and its validity if it has any
int plan_parent(Plan& P, ColPlan& cp, orcgpu_staged* s) {
  const orcgpu_column& c = cp.c;
  const int si = cp.stripe, ci = cp.col;
  if (c.parent) {
    const int pt = c.parent <= (uint32_t)ci ? s->cols[c.parent - 1].orc_type : -1;
    if (pt != ORCGPU_T_STRUCT && pt != ORCGPU_T_UNION) {
      set_err(s->ctx, "column %u: its parent must be a STRUCT or UNION column given before it (elements of Lists and Maps are decoded in a pass of their own)", c.column_id);
      return ORCGPU_INVALID_ARGUMENT;
    }
    for (int k = (int)P.cols.size() - 1; k >= 0; k--)
      if (P.cols[k].stripe == si && P.cols[k].col == (int)c.parent - 1) {
        if (pt == ORCGPU_T_UNION) {
          // the child of a Union stands below the ARM its position among the Union's children names
          int ordinal = 0;
          for (int q = (int)c.parent; q < ci; q++) ordinal += s->cols[q].parent == c.parent;
          if (ordinal >= P.cols[k].n_arms) {
            set_err(s->ctx, "column %u: the Union above it has more than 127 children", c.column_id);
            return ORCGPU_UNSUPPORTED;
          }
          k = P.cols[k].arm0 + ordinal;
        }
        cp.depth = P.cols[k].depth + 1;
        if (P.cols[k].has_present) cp.parent_plan = k;
        break;
      }
    if (cp.depth > kMaxStructDepth) {
      set_err(s->ctx, "column %u: Structs / Unions nested more than %d levels deep are not decoded on the GPU path", c.column_id, kMaxStructDepth);
      return ORCGPU_UNSUPPORTED;
    }
  }
  return ORCGPU_OK;
}

// PRESENT (PresentDecoder::from_stripe: get_opt -> only when the stream exists)
int plan_present(Plan& P, ColPlan& cp, orcgpu_staged* s, orcgpu_result* r) {
  const orcgpu_column& c = cp.c;
  const uint64_t n = cp.n_rows;
  const int si = cp.stripe, ci = cp.col;
  ColumnOut& co = r->cols[ci];
  Bump& RB = P.result_bump[si];
  cp.own_present = s->find(c.column_id, ORCGPU_S_PRESENT) != nullptr;
  cp.has_present = cp.own_present || cp.parent_plan >= 0;
  co.has_present = cp.has_present;
  if (cp.has_present && n) {
    take_validity_scratch(P, cp);
    if (cp.own_present) {
      cp.present = plan_stream(P, s, c.column_id, ORCGPU_S_PRESENT);
      cp.pbytes_off = P.scratch.take(cp.n_words * 8 + ORC_PAD + cp.present.skip_values);
      // bytes of the stream: ceil(rows / 8) -- of a Struct's field: of the rows in which the Struct is present, known on the
      // device only (the parent's scan leaves it in its ceil8 scalar; the fields' PRESENT jobs run behind it, by depth)
      // (entered at a row group in mid-byte: present.skip_bits bits of the first byte belong to the rows before.  The fields of one
      // Struct are entered at the same bit -- their streams count the same rows --: the Struct's scalar allows for it)
      const uint32_t bo = cp.present.skip_bits;
      if (cp.parent_plan >= 0) {
        ColPlan& pp = P.cols[cp.parent_plan];
        if (pp.child_bits_set && pp.child_bits != bo) {
          set_err(s->ctx, "column %u: its PRESENT stream is entered at bit %u, another field's of the same Struct at bit %u", c.column_id, bo, pp.child_bits);
          return ORCGPU_INVALID_ARGUMENT;
        }
        pp.child_bits = bo;
        pp.child_bits_set = true;
      }
      const uint32_t need = cp.parent_plan >= 0 ? P.cols[cp.parent_plan].ceil8_idx : P.new_scalar((n + bo + 7) / 8);
      const int cls = cp.parent_plan >= 0 ? JC_PRESENT1 + cp.depth - 1 : JC_PRESENT;
      cp.job_present = add_job(P, cls, CODEC_BYTE, false, 8, 1, cp.present, need, (n + bo + 7) / 8, si, ci, ORCGPU_S_PRESENT);
      P.jobs[cp.job_present].out_scratch_off = cp.pbytes_off;
      cp.pbytes_off += cp.present.skip_values;  // (a stream entered at a row group: the column's bytes lie behind those of the rows before)
    }
    co.validity_off = RB.take((uint64_t)r->n_batches * r->words_per_batch * 8);
  }
  return ORCGPU_OK;
}

int plan_union(Plan& P, ColPlan& cp, orcgpu_staged* s, orcgpu_result* r) {
  const orcgpu_column& c = cp.c;
  const uint64_t n = cp.n_rows;
  const int si = cp.stripe, ci = cp.col;
  ColumnOut& co = r->cols[ci];
  Bump& RB = P.result_bump[si];
  // union.rs:69-136: DATA = byte-RLE tags, one per row in which the Union is present; the result's values are the type ids (0 in
  // null rows: decode_spaced), the arms follow as plans of their own.  The tags are needed before the arms' validity can be
  // formed: their job is expanded with the PRESENT streams of the arms' depth.
  int n_arms = 0;
  for (size_t q = (size_t)ci + 1; q < s->cols.size(); q++) n_arms += s->cols[q].parent == (uint32_t)ci + 1;
  if (cp.depth + 1 > kMaxStructDepth || n_arms > 127) {
    set_err(s->ctx, "column %u: a Union %s is not decoded on the GPU path", c.column_id, n_arms > 127 ? "of more than 127 types" : "this deep inside Structs / Unions");
    return ORCGPU_UNSUPPORTED;
  }
  co.width = 1;
  co.values_bytes = n;
  co.values_off = RB.take(n + 16);
  if (n) {
    cp.data = plan_stream(P, s, c.column_id, ORCGPU_S_DATA);
    const uint64_t lead = cp.data.skip_values;
    cp.job_data = add_job(P, JC_PRESENT1 + cp.depth, CODEC_BYTE, false, 8, 1, cp.data, cp.nonnull_idx, n, si, ci, ORCGPU_S_DATA);
    place_dense(P, cp, co, n + 16 + lead + ORC_PAD, lead, false);
  }
  cp.arm0 = (int)P.cols.size() + 1;
  cp.n_arms = n_arms;
  const int me = (int)P.cols.size();
  P.cols.push_back(cp);
  for (int a = 0; a < n_arms; a++) {
    ColPlan arm{};
    arm.stripe = si;
    arm.col = -1;
    arm.c = c;
    arm.c.orc_type = ORCGPU_T_STRUCT;  // (towards its child it is what a Struct is towards a field)
    arm.n_rows = n;
    arm.has_present = true;
    arm.parent_plan = cp.has_present ? me : -1;
    arm.depth = cp.depth + 1;
    arm.arm_of = me;
    arm.arm_tag = a;
    arm.err_idx = P.new_scalar(RLE_NO_ERR);
    arm.nonnull_idx = P.new_scalar(n);
    arm.ceil8_idx = P.new_scalar((n + 7) / 8);
    arm.nullcount_off = (uint32_t)P.n_nullcount_slots;
    P.n_nullcount_slots += r->n_batches;
    if (n) {
      take_validity_scratch(P, arm);
      arm.arm_validity_off = P.scratch.take((uint64_t)r->n_batches * r->words_per_batch * 8 + 16);
    }
    P.cols.push_back(arm);
  }
  return ORCGPU_OK;
}

// The value streams of every other kind of column, their jobs and where those write
int plan_values(Plan& P, ColPlan& cp, orcgpu_staged* s, orcgpu_result* r) {
  const orcgpu_column& c = cp.c;
  const uint64_t n = cp.n_rows;
  const int si = cp.stripe, ci = cp.col;
  ColumnOut& co = r->cols[ci];
  Bump& RB = P.result_bump[si];
  // a writer time zone: values are re-labelled behind the finisher (tz_shift_kernel); only the ns unit of a zone that never
  // leaves UTC cannot produce nulls and is left alone
  if (c.orc_type == ORCGPU_T_TIMESTAMP && s->zone && n && !(s->zone->table.utc && co.ts_unit >= 3)) {
    cp.tz = true;
    if (co.ts_unit != 4 && !cp.has_present) {
      co.validity_off = RB.take((uint64_t)r->n_batches * r->words_per_batch * 8);
      co.has_present = true;  // the result carries validity words
    }
  }

  const int vcls = version_class(c);
  const int t = c.orc_type;
  if (!n) {
    // (no rows -- the elements of Lists that are all empty, an empty Map: nothing to decode, but the column keeps its kind: a List
    // without rows is still a List to whoever exports it)
    if (t == ORCGPU_T_LIST || t == ORCGPU_T_MAP) {
      co.is_list = true;
      co.is_map = t == ORCGPU_T_MAP;
    }
    P.cols.push_back(cp);
    return ORCGPU_OK;
  }
  if (t == ORCGPU_T_SHORT || t == ORCGPU_T_INT || t == ORCGPU_T_LONG || t == ORCGPU_T_DATE || t == ORCGPU_T_BYTE) {
    const int cls = t == ORCGPU_T_BYTE ? JC_BYTE : vcls;  // (a Byte column: byte RLE whatever its encoding, unsigned)
    cp.data = plan_stream(P, s, c.column_id, ORCGPU_S_DATA);
    const uint64_t lead = (uint64_t)cp.data.skip_values * co.width;  // values of the rows before an entry point: decoded in front
    co.values_bytes = n * co.width;
    co.values_off = RB.take(co.values_bytes + 16 + (cp.has_present ? 0 : lead));
    cp.job_data = add_job(P, cls, class_codec(cls), t != ORCGPU_T_BYTE, (uint8_t)(co.width * 8), (uint8_t)co.width, cp.data, cp.nonnull_idx, n, si, ci, ORCGPU_S_DATA);
    place_dense(P, cp, co, co.values_bytes + 16 + lead, lead, !cp.has_present);
  } else if (t == ORCGPU_T_BOOLEAN) {
    cp.data = plan_stream(P, s, c.column_id, ORCGPU_S_DATA);
    co.values_bytes = (uint64_t)r->n_batches * r->words_per_batch * 8;
    co.values_off = RB.take(co.values_bytes + 16);
    // needed bytes of the bit stream = ceil(non-null / 8): computed on the device into its own scalar
    uint32_t need = P.new_scalar((n + cp.data.skip_bits + 7) / 8);
    cp.dictbytes_idx = need;  // reused slot: "bytes needed" scalar for the boolean DATA job
    cp.dense_off = P.scratch.take((n + 7) / 8 + 1 + ORC_PAD + cp.data.skip_values);
    cp.job_data = add_job(P, JC_BYTE, CODEC_BYTE, false, 8, 1, cp.data, need, (n + cp.data.skip_bits + 7) / 8, si, ci, ORCGPU_S_DATA);
    P.jobs[cp.job_data].out_scratch_off = cp.dense_off;
    cp.dense_off += cp.data.skip_values;
  } else if (t == ORCGPU_T_FLOAT || t == ORCGPU_T_DOUBLE) {
    cp.data = plan_stream(P, s, c.column_id, ORCGPU_S_DATA);
    co.values_bytes = n * co.width;
    co.values_off = RB.take(co.values_bytes + 16);
  } else if (t == ORCGPU_T_TIMESTAMP || t == ORCGPU_T_TIMESTAMP_INSTANT) {
    cp.data = plan_stream(P, s, c.column_id, ORCGPU_S_DATA);
    cp.secondary = plan_stream(P, s, c.column_id, ORCGPU_S_SECONDARY);
    if (co.ts_unit == 4) co.width = 16;  // Decimal128(38, 9)
    co.values_bytes = n * co.width;
    co.values_off = RB.take(co.values_bytes + 16, 256);
    cp.dense_off = P.scratch.take(n * 8 + 16 + 8ull * cp.data.skip_values);
    cp.dense2_off = P.scratch.take(n * 8 + 16 + 8ull * cp.secondary.skip_values);
    cp.job_data = add_job(P, vcls, class_codec(vcls), true, 64, 8, cp.data, cp.nonnull_idx, n, si, ci, ORCGPU_S_DATA);
    P.jobs[cp.job_data].out_scratch_off = cp.dense_off;
    cp.dense_off += 8ull * cp.data.skip_values;
    cp.job_secondary = add_job(P, vcls, class_codec(vcls), false, 64, 8, cp.secondary, cp.nonnull_idx, n, si, ci, ORCGPU_S_SECONDARY);
    P.jobs[cp.job_secondary].out_scratch_off = cp.dense2_off;
    cp.dense2_off += 8ull * cp.secondary.skip_values;
  } else {
    int st = plan_column_ext(P, cp, co, s, r, vcls);
    if (st) return st;
  }
  P.cols.push_back(cp);
  return ORCGPU_OK;
}

// ---- plan -------------------------------------------------------------------------------------
int plan_columns(LaneRun& R) {
  Plan& P = R.P;
  P.lane_id = R.ctx->lane_id;
  P.call_z_lanes = R.ctx->call_z_lanes;
  P.result_bump.resize(R.n);
  for (uint32_t si = 0; si < R.n; si++) {
    orcgpu_staged* s = R.stripes[si];
    orcgpu_result* r = R.results[si];
    P.stripes.push_back(s);
    P.results.push_back(r);
    for (size_t ci = 0; ci < s->cols.size(); ci++) {
      if (R.mask && !(*R.mask)[si][ci]) continue;
      if (r->cols[ci].elem) continue;  // an element of a List / Map: decoded with its siblings once their count is known
      int rc = plan_column(P, (int)si, (int)ci, s, r);
      if (rc) {
        if (R.ctx != s->ctx) R.ctx->err = s->ctx->err;  // plan_column reports to the staging context
        return rc;
      }
    }
    if (int rc = lookup_plan_stripe(R, si)) return rc;
    if (int rc = computed_plan_stripe(R, si)) return rc;
  }
  R.ht.cols = host_us_now();
  return ORCGPU_OK;
}

// compressed streams: chunk tables
int plan_chunk_tables(LaneRun& R) {
  int rc = plan_decompress(R.P, R.DP);
  R.ht.dp = host_us_now();
  return rc;
}

int lay_out_jobs(LaneRun& R) {
  R.L = layout_jobs(R.P.jobs);
  R.njobs = (int)R.L.order.size();
  if (R.L.fits) return ORCGPU_OK;
  set_err(R.ctx, "stripe batch too large: %llu stream blocks", (unsigned long long)R.L.total_blocks);
  return ORCGPU_INVALID_ARGUMENT;
}

// The workspace of everything behind the plan -- the per-block arrays, the exact walk's maps, the hint table, the summary and
// the job tables of the later phases --, then the memory itself: workspace, result arenas, pinned summary.
int reserve_workspace(LaneRun& R) {
  orcgpu_ctx* const ctx = R.ctx;
  Plan& P = R.P;
  const uint64_t total_blocks = R.L.total_blocks, n_tiles = R.L.n_tiles;
  auto& B = R.blk_off;
  B.entry = P.scratch.take(total_blocks * 4), B.exit_ = P.scratch.take(total_blocks * 4);
  B.nvals = P.scratch.take(total_blocks * 4), B.voff = P.scratch.take(total_blocks * 4);
  B.tbase = P.scratch.take(n_tiles * 4 + 16), B.tsum = P.scratch.take(n_tiles * 4 + 16);
  B.flags = P.scratch.take(total_blocks + 16);
  B.badmap = P.scratch.take(total_blocks / 8 + 64);
  B.gjob = P.scratch.take((uint64_t)R.L.cls_tab0[JC_COUNT] * 4 + 16);
  // the exact parallel walk (rle_exact_*): a map of 4608 two-byte exits per span of 256 blocks and per tile, 7 % of the streams' bytes
  R.n_xspans = (uint32_t)((total_blocks + RLE_EXACT_SPAN - 1) / RLE_EXACT_SPAN);
  // The exact parallel walk -- four launches, two of them of 512-thread workgroups with 51 KiB of LDS that "end at once" for
  // streams that do not need them -- is only sent when the LAST call of this lane met a stream that did (orcgpu_ctx::exact_on:
  // a job whose mending passes left RLE_EXACT_MIN blocks or more).  Ending at once is not free: beside the other column lane's
  // expansion kernel such a workgroup waits until eight wavefront slots and its LDS are free on one CU -- 4.1 ms in the queue in
  // one headline step, the lane's expansion behind it (rocprof, round 6).  A stream of that kind met for the first time goes
  // through the serial repair once (exact either way; 23 instead of 3.6 ms per 24 M rows of bench.py's c2-adv), the calls behind
  // it -- the next stripes of the same file -- take the parallel walk.
  R.use_exact = total_blocks >= 2048 && ctx->exact_on;  // (smaller calls: the serial repair is quick enough)
  if (R.use_exact) {
    R.x_fmap = P.scratch.take((uint64_t)R.n_xspans * RLE_EXACT_E * 2 + 16);
    R.x_gmap = P.scratch.take(n_tiles * RLE_EXACT_E * 2 + 16);
    R.x_tile = P.scratch.take(n_tiles * 4 + 16);
    R.x_span = P.scratch.take((uint64_t)R.n_xspans * 4 + 16);
  }
  // verified run starts (orcgpu_stream::entries): one table for the call, a slice per job; the per-block entries they give
  for (size_t k = 0; k < R.L.order.size(); k++) {
    const JobPlan& j = P.jobs[R.L.order[k]];
    if (!j.hint_src) continue;
    for (auto& h : j.hint_src->hints) R.hints.push_back(RleHint{(uint32_t)k, h.first == 0xffffffffu ? 0xffffffffu : j.chunk0 + h.first, h.second, 0});
  }
  R.hints_off = R.hints.empty() ? 0 : P.scratch.take(R.hints.size() * sizeof(RleHint) + 16);
  B.hint = R.hints.empty() ? 0 : P.scratch.take(total_blocks * 4 + 16);

  SummaryLayout& SL = R.SL;
  {
    Bump sb;
    SL.scalars_off = sb.take(P.scalars.size() * 8 + 8, 16);
    SL.jobs_off = sb.take(P.jobs.size() * sizeof(RleJob) + 16, 16);
    SL.nullc_off = sb.take(P.n_nullcount_slots * 8 + 8, 16);
    SL.chartot_off = sb.take(P.n_chartot_slots * 8 + 8, 16);
    SL.bytes = align_up(sb.off, 16);
  }
  R.summary_off = P.scratch.take(SL.bytes);
  {
    size_t ndict = 0;
    for (auto& cp : P.cols) ndict += cp.is_dict ? 1 : 0;
    P.dictjobs_off = P.scratch.take(ndict * sizeof(DictJob) + 64);
    P.dictplaces_off = P.scratch.take(R.n * sizeof(DictPlace) + 64);
    size_t npres = 0;
    for (auto& cp : P.cols) npres += cp.has_present ? 1 : 0;
    P.presjobs_off = P.scratch.take(npres * sizeof(PresJob) + 64);
    P.spacejobs_off = P.scratch.take(npres * sizeof(SpaceJob) + 64);
  }
  {
    // finisher job table (FinBatch): at most a dozen small launches per column
    P.finjobs_cap = (uint64_t)P.cols.size() * 16 * sizeof(MJob) + 1024;
    P.finjobs_off = P.scratch.take(P.finjobs_cap, 16);
  }

  // ---- memory ------------------------------------------------------------------------------------------
  (void)hipStreamSynchronize(R.st);  // earlier work may still use scratch / pinned memory
  ctx->upload_reset();
  if (!ctx->scratch.ensure(P.scratch.off + kAlign)) {
    set_err(ctx, "hipMalloc(%llu) for the decode workspace failed", (unsigned long long)P.scratch.off);
    return ORCGPU_HIP_ERROR;
  }
  for (uint32_t si = 0; si < R.n; si++) {
    P.results[si]->arena_used[ctx->lane_id] = P.result_bump[si].off;
    P.results[si]->chars_used[ctx->lane_id] = 0;
    if (!P.results[si]->arena[ctx->lane_id].ensure(P.result_bump[si].off + kAlign)) {
      set_err(ctx, "hipMalloc(%llu) for the result buffers failed", (unsigned long long)P.result_bump[si].off);
      return ORCGPU_HIP_ERROR;
    }
  }
  if (!ctx->ensure_pinned(SL.bytes + R.DP.table_bytes + 64)) {
    set_err(ctx, "hipHostMalloc for the summary failed");
    return ORCGPU_HIP_ERROR;
  }
  R.S = ctx->scratch.p;
  {
    // debugging aid (tests / fuzzing): fill the workspace and the result buffers with a byte pattern so that
    // anything read before it is written shows up deterministically instead of depending on earlier decodes
    static const char* poison = getenv("ORCGPU_POISON");
    if (poison && *poison) {
      const int v = (int)strtol(poison, nullptr, 0) & 0xFF;
      (void)hipMemsetAsync(R.S, v, P.scratch.off, R.st);
      for (uint32_t si = 0; si < R.n; si++) (void)hipMemsetAsync(R.arena(P.results[si]), v, P.result_bump[si].off, R.st);
    }
  }
  return ORCGPU_OK;
}

// ---- host mirror of the summary, and where its device copy and the block arrays lie -----------------------------------------
void fill_summary_mirror(LaneRun& R) {
  const Plan& P = R.P;
  const JobLayout& L = R.L;
  const SummaryLayout& SL = R.SL;
  uint8_t* const S = R.S;
  uint8_t* const hs = R.hs = R.ctx->pinned;
  memset(hs, 0, SL.bytes);
  memcpy(hs + SL.scalars_off, P.scalars.data(), P.scalars.size() * 8);
  RleJob* const hjobs = R.hjobs = reinterpret_cast<RleJob*>(hs + SL.jobs_off);
  for (size_t k = 0; k < L.order.size(); k++) {
    const JobPlan& j = P.jobs[L.order[k]];
    RleJob& d = hjobs[k];
    d.data = j.data_scratch_off != ~0ull ? S + j.data_scratch_off : j.data;
    d.out = j.out_result_off != ~0ull ? (void*)(R.arena(P.results[j.result_index]) + j.out_result_off) : (void*)(S + j.out_scratch_off);
    d.len_idx = j.len_idx;
    d.needed_idx = j.needed_idx;
    d.total_idx = j.total_idx;
    d.block0 = j.block0;
    d.nblocks = j.nblocks;
    d.group0 = j.group0;
    d.ngroups = j.ngroups;
    d.group_size = j.group_size;
    d.group_tab0 = L.cls_tab0[j.cls] + j.group0;
    d.class_index = (uint32_t)j.final_index - L.cls_first[j.cls];
    d.codec = j.codec;
    d.is_signed = j.is_signed;
    d.nbits = j.nbits;
    d.out_bytes = j.out_bytes;
    d.first_bad = 0xffffffffu;
    d.stat_bad = 0;
    d.stat_repaired = 0;
    d.skip = j.skip_values;
    d.bad_left = 0;
    d.hint0 = d.n_hints = d.hint_bad = 0;
    d.hint_skip = j.hint_src ? j.hint_src->skip_bytes : 0;
    d.uniform_idx = j.uniform_idx;
    d.uniform_value = j.uniform_value;
    d.err = RLE_NO_ERR;
    d.err_pos = RLE_NO_ERR;
  }
  for (size_t h = 0; h < R.hints.size(); h++) {
    RleJob& d = hjobs[R.hints[h].job];
    if (!d.n_hints) d.hint0 = (uint32_t)h;
    d.n_hints++;
  }
  uint8_t* const dsum = R.dsum = S + R.summary_off;
  R.d_scalars = reinterpret_cast<uint64_t*>(dsum + SL.scalars_off);
  R.d_jobs = reinterpret_cast<RleJob*>(dsum + SL.jobs_off);
  R.d_nullc = reinterpret_cast<unsigned long long*>(dsum + SL.nullc_off);
  R.d_chartot = reinterpret_cast<unsigned long long*>(dsum + SL.chartot_off);
  RleBlocks& blk = R.blk;
  const auto& B = R.blk_off;
  blk.entry = reinterpret_cast<uint32_t*>(S + B.entry);
  blk.exit_ = reinterpret_cast<uint32_t*>(S + B.exit_);
  blk.nvals = reinterpret_cast<uint32_t*>(S + B.nvals);
  blk.voff = reinterpret_cast<uint32_t*>(S + B.voff);
  blk.tile_base = reinterpret_cast<uint32_t*>(S + B.tbase);
  blk.flags = S + B.flags;
  blk.badmap = reinterpret_cast<uint32_t*>(S + B.badmap);
  blk.group_job = reinterpret_cast<uint32_t*>(S + B.gjob);
  blk.hint = R.hints.empty() ? nullptr : reinterpret_cast<uint32_t*>(S + B.hint);
  R.d_tsum = reinterpret_cast<uint32_t*>(S + B.tsum);
}

// ---- launches ------------------------------------------------------------------------------------------
int launch_decompression(LaneRun& R) {
  orcgpu_ctx* const ctx = R.ctx;
  hipStream_t st = R.st;
  R.ht.plan = host_us_now();
  for (uint32_t si = 0; si < R.n; si++)  // the stripes' bytes may still be on their way (staging does not wait for its copies)
    if (R.stripes[si]->ready) HIP_TRY(ctx, hipStreamWaitEvent(st, R.stripes[si]->ready, 0));
  HIP_TRY(ctx, hipEventRecord(ctx->ev[0], st));
  ctx->kev_used[0] = ctx->kev_used[1] = false;
  ctx->lit_ev_used = false;
  HIP_TRY(ctx, hipMemcpyAsync(R.dsum, R.hs, R.SL.bytes, hipMemcpyHostToDevice, st));
  R.ht.launch = host_us_now();  // (the waits for the stripes' bytes and the summary's copy are enqueued)
  ctx->hp_fill = ctx->hp_upload = ctx->hp_gate = 0;
  int rc = launch_decompress(ctx, R.P, R.DP, R.S, R.d_scalars, R.hs + R.SL.bytes, ctx->ev[6], ctx->ev[7], ctx->ev[4], ctx->ev[8]);
  R.ht.first = host_us_now();
  return rc;
}

// The per-block entries the hints give, the block walk with its mending passes, the repair and the scans of the values per block
int launch_walk(LaneRun& R) {
  orcgpu_ctx* const ctx = R.ctx;
  hipStream_t st = R.st;
  uint8_t* const S = R.S;
  RleJob* const d_jobs = R.d_jobs;
  uint64_t* const d_scalars = R.d_scalars;
  const RleBlocks& blk = R.blk;
  const std::vector<RleHint>& hints = R.hints;
  const uint64_t total_blocks = R.L.total_blocks;
  const uint32_t n_tiles = R.L.n_tiles, n_xspans = R.n_xspans;
  const int njobs = R.njobs;
  if (njobs && !hints.empty()) {
    HIP_TRY(ctx, hipMemsetAsync(blk.hint, 0xff, total_blocks * 4, st));
    HIP_TRY(ctx, ctx->upload(S + R.hints_off, hints.data(), hints.size() * sizeof(RleHint), st));
    HIP_TRY(ctx, launch(rle_hint_kernel, (uint64_t)hints.size(), false, 64, st, d_jobs, (const RleHint*)(S + R.hints_off), (uint32_t)hints.size(), blk,
                        (const uint64_t*)d_scalars, (const uint32_t*)(R.DP.n_chunks ? S + R.DP.chunk_start_off : S)));
  }
  if (njobs) {
    static const int kModes[] = {0, 3, -1, 1, 1, 2};  // guess, fill, short-run spans, relax x2 (4 sweeps each), verify
    for (int mode : kModes) {
      if (mode < 0)
      {
        // spans (64 blocks) per workgroup: 1 for small batches, up to 8 once there are thousands of spans
        uint32_t spw = 1;
        // (2048: with 512 -- more spans per workgroup, more of them entered with the exit carried on from the span before instead of a
        // warm-up -- C3's walk took 0.49 instead of 0.41 ms and lineitem SF 4's 2.13 instead of 1.73: fewer workgroups cost more)
        while (spw < 8 && total_blocks / (64ull * spw * 2) >= 2048) spw *= 2;
        if (!ctx->kev_used[0]) HIP_TRY(ctx, hipEventRecord(ctx->kev[0][0], st));
        HIP_TRY(ctx, launch(rle_walk_short_kernel, (total_blocks + 64ull * spw - 1) / (64ull * spw), true, 64 * RLE_SHORT_WAVES, st, d_jobs, njobs, blk,
                            (const uint64_t*)d_scalars, (uint32_t)total_blocks, spw));
        HIP_TRY(ctx, hipEventRecord(ctx->kev[0][1], st));
        ctx->kev_used[0] = true;
      }
      else
        HIP_TRY(ctx, launch(rle_walk_kernel, total_blocks, false, 64, st, d_jobs, njobs, blk, (const uint64_t*)d_scalars, (uint32_t)total_blocks, mode));
    }
    for (int pass = 0; pass < 2; pass++) {
      // damaged stretches, all at once; then the check again (both return at once for streams the first check passed)
      HIP_TRY(ctx, launch(rle_mend_kernel, total_blocks, false, 256, st, d_jobs, njobs, blk, (const uint64_t*)d_scalars, (uint32_t)total_blocks));
      HIP_TRY(ctx, launch(rle_walk_kernel, total_blocks, false, 64, st, d_jobs, njobs, blk, (const uint64_t*)d_scalars, (uint32_t)total_blocks, 5));
    }
    if (R.use_exact) {
      // streams the mending passes could not settle: the exact walk, in parallel (four launches that end at once otherwise)
      uint16_t* fmap = reinterpret_cast<uint16_t*>(S + R.x_fmap);
      uint16_t* gmap = reinterpret_cast<uint16_t*>(S + R.x_gmap);
      uint32_t* tile_e = reinterpret_cast<uint32_t*>(S + R.x_tile);
      uint32_t* span_e = reinterpret_cast<uint32_t*>(S + R.x_span);
      const uint64_t cus = ctx->n_cus ? ctx->n_cus : 256;
      HIP_TRY(ctx, launch(rle_exact_map_kernel, std::min<uint64_t>(n_xspans, 2 * cus), true, RLE_EXACT_WG, st, d_jobs, njobs, (const uint64_t*)d_scalars, (uint32_t)total_blocks, fmap));
      HIP_TRY(ctx, launch(rle_exact_tile_kernel, std::min<uint64_t>(n_tiles, 4 * cus), true, RLE_EXACT_WG, st, d_jobs, njobs, (const uint64_t*)d_scalars, (uint32_t)total_blocks,
                          (const uint16_t*)fmap, gmap));
      HIP_TRY(ctx, launch(rle_exact_chain_kernel, (uint64_t)njobs, true, 64, st, d_jobs, njobs, (const uint64_t*)d_scalars, (const uint16_t*)fmap, (const uint16_t*)gmap, tile_e, span_e));
      HIP_TRY(ctx, launch(rle_exact_fill_kernel, std::min<uint64_t>(n_xspans, 2 * cus), true, RLE_EXACT_WG, st, d_jobs, njobs, blk, (const uint64_t*)d_scalars, (uint32_t)total_blocks,
                          (const uint32_t*)span_e));
    }
    HIP_TRY(ctx, launch(rle_repair_kernel, (uint64_t)njobs, true, 64, st, d_jobs, njobs, blk, (const uint64_t*)d_scalars));
    HIP_TRY(ctx, launch(rle_tile_scan_kernel, (uint64_t)n_tiles, true, 256, st, blk, R.d_tsum));
    HIP_TRY(ctx, launch(rle_job_scan_kernel, (uint64_t)njobs, true, 256, st, (const RleJob*)d_jobs, blk, (const uint32_t*)R.d_tsum, d_scalars));
  }
  HIP_TRY(ctx, hipEventRecord(ctx->ev[5], st));
  R.ht.walk = host_us_now();
  return ORCGPU_OK;
}

// One class's expansion: a wavefront per group of blocks
template <typename K>
hipError_t launch_expand(LaneRun& R, K kernel, int cls, uint32_t* launches = nullptr) {
  const JobLayout& L = R.L;
  if (!L.cls_groups[cls]) return hipSuccess;
  const hipError_t e = launch(kernel, (uint64_t)(L.cls_groups[cls] + 3) / 4, true, 256, R.st, R.d_jobs + L.cls_first[cls], (const uint32_t*)(R.blk.group_job + L.cls_tab0[cls]),
                              R.blk, (const uint64_t*)R.d_scalars, L.cls_groups[cls]);
  if (e == hipSuccess && launches) ++*launches;  // (orcgpu_last_timing counts the launches of the expansion phase)
  return e;
}

// The PRESENT job of a column, or of a Union's arm: where its bits come from and what is formed of them
PresJob make_pres_job(LaneRun& R, const ColPlan& cp) {
  const Plan& P = R.P;
  uint8_t* const S = R.S;
  uint64_t* const d_scalars = R.d_scalars;
  orcgpu_result* r = P.results[cp.stripe];
  PresJob j{};
  const ColPlan* above = nullptr;  // the Struct / Union / arm whose non-null rows this one's bits are dealt out to
  if (cp.arm_of >= 0) {
    // an arm of a Union: valid where the Union is and its tag is the arm's
    const ColPlan& un = P.cols[cp.arm_of];
    j.tags = reinterpret_cast<const int8_t*>(S + un.dense_off);
    j.tag = cp.arm_tag;
    j.validity = reinterpret_cast<unsigned long long*>(S + cp.arm_validity_off);
    j.ceil8b_out = d_scalars + cp.ceil8_idx;
    if (un.has_present) above = &un;
  } else {
    ColumnOut& co = r->cols[cp.col];
    j.pbytes = cp.own_present ? S + cp.pbytes_off : nullptr;
    j.validity = reinterpret_cast<unsigned long long*>(R.arena(r) + co.validity_off);
    j.ceil8_out = cp.c.orc_type == ORCGPU_T_BOOLEAN ? d_scalars + cp.dictbytes_idx : nullptr;
    j.ceil8b_out = cp.c.orc_type == ORCGPU_T_STRUCT ? d_scalars + cp.ceil8_idx : nullptr;
    j.bit0 = cp.own_present ? cp.present.skip_bits : 0;
    j.data_bits = cp.c.orc_type == ORCGPU_T_BOOLEAN ? cp.data.skip_bits : 0;
    j.job = cp.own_present ? R.d_jobs + P.jobs[cp.job_present].final_index : nullptr;
    if (cp.parent_plan >= 0) above = &P.cols[cp.parent_plan];
  }
  j.child_bits = cp.child_bits;  // (its child's PRESENT stream entered in mid-byte: a Union in a stripe read by row groups)
  j.vbits = reinterpret_cast<unsigned long long*>(S + cp.vbits_off);
  j.wpop = reinterpret_cast<uint32_t*>(S + cp.wpop_off);
  j.rank = reinterpret_cast<uint32_t*>(S + cp.rank_off);
  j.rtiles = reinterpret_cast<uint32_t*>(S + cp.rank_tiles_off);
  j.null_counts = R.d_nullc + cp.nullcount_off;
  j.nonnull_out = d_scalars + cp.nonnull_idx;
  if (above) {
    j.parent_vbits = reinterpret_cast<const unsigned long long*>(S + above->vbits_off);
    j.parent_rank = reinterpret_cast<const uint32_t*>(S + above->rank_off);
  }
  j.n_rows = cp.n_rows;
  j.n_words = cp.n_words;
  j.n_rank_tiles = cp.n_rank_tiles;
  j.n_out_words = (uint64_t)r->n_batches * r->words_per_batch;
  j.batch = r->batch;
  j.words_per_batch = r->words_per_batch;
  return j;
}

// PRESENT streams first: everything else needs the non-null counts.  By depth: the PRESENT stream of a Struct's field is as
// long as the Struct has non-null rows, and its bits are dealt out to them (array_decoder/mod.rs:216-252): depth d needs the
// words, ranks and counts of depth d - 1.
int launch_present(LaneRun& R) {
  orcgpu_ctx* const ctx = R.ctx;
  hipStream_t st = R.st;
  Plan& P = R.P;
  size_t pres_at = 0;  // presjobs of the depths done so far (the device table is filled depth after depth)
  P.presjobs.reserve(P.cols.size());
  PresJob* const dp_all = reinterpret_cast<PresJob*>(R.S + P.presjobs_off);
  P.presjobs.clear();
  int max_depth = 0;
  for (auto& cp : P.cols) max_depth = std::max(max_depth, cp.depth);
  for (int depth = 0; depth <= max_depth && depth <= kMaxStructDepth; depth++) {
    HIP_TRY(ctx, launch_expand(R, byte_expand_kernel, depth == 0 ? JC_PRESENT : JC_PRESENT1 + depth - 1));
    // validity words, ranks, per-batch bitmaps and null counts of ALL columns of this depth: five launches
    uint64_t max_words = 0, max_tiles = 0, max_out = 0;
    for (auto& cp : P.cols) {
      if (!cp.has_present || cp.depth != depth || !cp.n_rows) continue;
      const PresJob j = make_pres_job(R, cp);
      P.presjobs.push_back(j);
      max_words = std::max<uint64_t>(max_words, j.n_words);
      max_tiles = std::max<uint64_t>(max_tiles, j.n_rank_tiles);
      max_out = std::max<uint64_t>(max_out, j.n_out_words);
    }
    const uint32_t np = (uint32_t)(P.presjobs.size() - pres_at);
    if (np) {
      PresJob* dp = dp_all + pres_at;
      HIP_TRY(ctx, ctx->upload(dp, P.presjobs.data() + pres_at, np * sizeof(PresJob), st));
      // (grid.y is limited to 65535: more columns than that go in slices)
      for (uint32_t o = 0; o < np; o += 65535u) {
        const uint32_t ny = std::min<uint32_t>(65535u, np - o);
        const PresJob* dq = dp + o;
        auto grid = [&](uint64_t threads) { return dim3((uint32_t)std::max<uint64_t>(1, (threads + 255) / 256), ny); };
        hipLaunchKernelGGL(pres_words_kernel, grid(max_words), dim3(256), 0, st, dq);
        hipLaunchKernelGGL(pres_scan_tiles_kernel, dim3((uint32_t)std::max<uint64_t>(1, max_tiles), ny), dim3(256), 0, st, dq);
        hipLaunchKernelGGL(pres_scan_sums_kernel, dim3(ny), dim3(256), 0, st, dq);
        hipLaunchKernelGGL(pres_scan_apply_kernel, grid(max_words), dim3(256), 0, st, dq);
        hipLaunchKernelGGL(pres_validity_kernel, grid(max_out), dim3(256), 0, st, dq);
      }
      HIP_TRY(ctx, hipGetLastError());
    }
    pres_at = P.presjobs.size();
  }
  HIP_TRY(ctx, hipEventRecord(ctx->ev[1], st));
  R.ht.pres = host_us_now();
  return ORCGPU_OK;
}

int launch_expansion(LaneRun& R) {
  orcgpu_ctx* const ctx = R.ctx;
  ctx->last_expand_launches = 0;
  {
    // streams expected to hold one value throughout (Decimal scales): checked in front of the expansion, which then skips them
    bool any_uniform = false;
    for (const JobPlan& j : R.P.jobs) any_uniform = any_uniform || j.uniform_idx != 0;
    if (any_uniform) HIP_TRY(ctx, launch(rle2_uniform_kernel, (uint64_t)R.njobs, true, 256, R.st, (const RleJob*)R.d_jobs, (uint32_t)R.njobs, R.d_scalars));
  }
  HIP_TRY(ctx, launch_expand(R, rle2_expand_kernel, JC_RLE2, &ctx->last_expand_launches));
  HIP_TRY(ctx, launch_expand(R, rle1_expand_kernel, JC_RLE1, &ctx->last_expand_launches));
  HIP_TRY(ctx, launch_expand(R, byte_expand_kernel, JC_BYTE, &ctx->last_expand_launches));
  HIP_TRY(ctx, hipEventRecord(ctx->ev[2], R.st));
  R.ht.exp = host_us_now();
  return ORCGPU_OK;
}

// ---- finishers: null spacing and per-type assembly -------------------------------------------------------
// One column's finisher launches, filed in `fin` by stage; its null spacing in P.spacejobs; its time zone shift in `tzjobs`
int file_finishers(LaneRun& R, FinBatch& fin, std::vector<TzJob>& tzjobs, ColPlan& cp) {
  Plan& P = R.P;
  uint8_t* const S = R.S;
  uint64_t* const d_scalars = R.d_scalars;
  if (cp.col < 0) return ORCGPU_OK;  // (an arm of a Union: no column of its own)
  orcgpu_result* r = P.results[cp.stripe];
  ColumnOut& co = r->cols[cp.col];
  const uint64_t nr = cp.n_rows;
  if (!nr) return ORCGPU_OK;
  const unsigned long long* vbits = R.vbits(cp);
  const uint32_t* rank = R.rank(cp);
  uint8_t* values = R.arena(r) + co.values_off;
  const int t = cp.c.orc_type;
  if (t == ORCGPU_T_UNION) {
    // the type ids: the dense tags spaced over the rows (0 where the Union is null), checked against the number of arms
    if (cp.has_present) P.spacejobs.push_back(SpaceJob{S + cp.dense_off, vbits, rank, values, nr, 1, 0, ~0ull});
    else fin.add<copy_bytes_body, 256>(0, (nr + 15) / 16, false, (const uint8_t*)(S + cp.dense_off), values, nr);
    fin.add<union_tags_body, 256>(0, nr, false, (const int8_t*)(S + cp.dense_off), (const uint64_t*)(d_scalars + cp.nonnull_idx), (int32_t)cp.n_arms,
                                  reinterpret_cast<unsigned long long*>(d_scalars + cp.err_idx));
  } else if (t == ORCGPU_T_SHORT || t == ORCGPU_T_INT || t == ORCGPU_T_LONG || t == ORCGPU_T_DATE || t == ORCGPU_T_BYTE) {
    if (cp.has_present) P.spacejobs.push_back(SpaceJob{S + cp.dense_off, vbits, rank, values, nr, co.width, 0, ~0ull});  // one launch for all, below
  } else if (t == ORCGPU_T_BOOLEAN) {
    uint64_t n_out = (uint64_t)r->n_batches * r->words_per_batch;
    fin.add<bool_values_body, 256>(0, n_out, false, (const uint8_t*)(S + cp.dense_off), vbits, rank, nr, r->batch, r->words_per_batch,
                                   reinterpret_cast<unsigned long long*>(values), n_out, cp.data.skip_bits);
  } else if (t == ORCGPU_T_FLOAT || t == ORCGPU_T_DOUBLE) {
    const uint8_t* src = cp.data.scratch_off != ~0ull ? S + cp.data.scratch_off : cp.data.dev;
    fin.add<float_check_body, 64>(0, 1, true, (const uint64_t*)d_scalars, cp.data.len_idx, cp.nonnull_idx, co.width, d_scalars + cp.err_idx);
    if (cp.has_present) {
      P.spacejobs.push_back(SpaceJob{src, vbits, rank, values, nr, co.width, 0, cp.data.len_upper / co.width});
    } else {
      uint64_t nb = std::min<uint64_t>(nr * co.width, cp.data.len_upper);
      fin.add<copy_bytes_body, 256>(0, (nb + 15) / 16, false, src, values, nb);
    }
  } else if (t == ORCGPU_T_TIMESTAMP || t == ORCGPU_T_TIMESTAMP_INSTANT) {
    fin.add<timestamp_body, 256>(0, nr, false, (const int64_t*)(S + cp.dense_off), (const int64_t*)(S + cp.dense2_off), vbits, rank, (int64_t*)values, nr,
                                 // TIMESTAMP_INSTANT is UTC whatever the writer's zone (timestamp.rs:88-93)
                                 t == ORCGPU_T_TIMESTAMP_INSTANT ? (int64_t)1420070400 : (int64_t)P.stripes[cp.stripe]->desc.ts_base_seconds, co.ts_unit,
                                 reinterpret_cast<unsigned long long*>(d_scalars + cp.err_idx));
    if (cp.tz) {
      const orcgpu_staged* sg = P.stripes[cp.stripe];
      const uint32_t n_at = (uint32_t)sg->zone->table.at.size();
      TzJob j{};
      j.values = values;
      j.vbits = vbits;
      j.validity = co.ts_unit != 4 ? reinterpret_cast<unsigned long long*>(R.arena(r) + co.validity_off) : nullptr;
      j.null_counts = R.d_nullc + cp.nullcount_off;
      j.at = reinterpret_cast<const long long*>(sg->zone->dev);
      j.offs = reinterpret_cast<const int*>(sg->zone->dev + (size_t)n_at * 8);
      j.n_rows = nr;
      j.n_at = n_at;
      j.offs0 = sg->zone->table.offs0;
      j.fold_at = sg->zone->table.fold_at;
      j.unit = co.ts_unit;
      j.batch = r->batch;
      j.words_per_batch = r->words_per_batch;
      if (!cp.has_present && co.ts_unit != 4) {
        const uint64_t nw = (uint64_t)r->n_batches * r->words_per_batch;
        fin.add<validity_ones_body, 256>(0, nw, false, j.validity, nr, r->batch, r->words_per_batch, nw);
      }
      tzjobs.push_back(j);  // (behind the timestamp finishers: launched after the batch below)
    }
  } else {
    return launch_finish_ext(R, fin, cp, co, r);
  }
  return ORCGPU_OK;
}

int launch_finishers(LaneRun& R) {
  orcgpu_ctx* const ctx = R.ctx;
  hipStream_t st = R.st;
  Plan& P = R.P;
  uint8_t* const S = R.S;
  P.spacejobs.clear();
  FinBatch fin;                 // the per-column finisher launches, filed by stage and sent together behind the loop
  std::vector<TzJob> tzjobs;
  for (auto& cp : P.cols)
    if (int rc = file_finishers(R, fin, tzjobs, cp)) return rc;
  if (fin.n_jobs) {
    // one upload of all job tables (pinned staging: the copy does not wait for the host), then one launch per stage and kernel
    const size_t bytes = fin.n_jobs * sizeof(MJob);
    if (bytes > P.finjobs_cap) {
      set_err(ctx, "finisher job table: %zu jobs do not fit the %llu bytes reserved", fin.n_jobs, (unsigned long long)P.finjobs_cap);
      return ORCGPU_UNEXPECTED;
    }
    if (bytes > ctx->fin_pinned_cap) {
      if (ctx->fin_pinned) (void)hipHostFree(ctx->fin_pinned);
      ctx->fin_pinned = nullptr;
      ctx->fin_pinned_cap = 0;
      HIP_TRY(ctx, hipHostMalloc((void**)&ctx->fin_pinned, bytes * 2, hipHostMallocDefault));
      ctx->fin_pinned_cap = bytes * 2;
    }
    std::stable_sort(fin.entries.begin(), fin.entries.end(), [](const FinBatch::Entry& a, const FinBatch::Entry& b) { return a.stage < b.stage; });
    MJob* hj = reinterpret_cast<MJob*>(ctx->fin_pinned);
    size_t k = 0;
    for (auto& e : fin.entries) {
      memcpy(hj + k, e.jobs.data(), e.jobs.size() * sizeof(MJob));
      k += e.jobs.size();
    }
    MJob* dj = reinterpret_cast<MJob*>(S + P.finjobs_off);
    HIP_TRY(ctx, hipMemcpyAsync(dj, hj, bytes, hipMemcpyHostToDevice, st));
    k = 0;
    for (auto& e : fin.entries) {
      e.launcher(dj + k, (uint32_t)e.jobs.size(), e.max_blocks, st);
      k += e.jobs.size();
    }
    HIP_TRY(ctx, hipGetLastError());
  }
  for (auto& j : tzjobs) HIP_TRY(ctx, launch(tz_shift_kernel, j.n_rows, false, 256, st, j));
  if (!P.spacejobs.empty()) {
    // null spacing of every fixed-width column with nulls: one launch
    const uint32_t ns = (uint32_t)P.spacejobs.size();
    SpaceJob* ds = reinterpret_cast<SpaceJob*>(S + P.spacejobs_off);
    uint64_t max_rows = 0;
    for (auto& j : P.spacejobs) max_rows = std::max(max_rows, j.n_rows);
    HIP_TRY(ctx, ctx->upload(ds, P.spacejobs.data(), ns * sizeof(SpaceJob), st));
    for (uint32_t o = 0; o < ns; o += 65535u)
      hipLaunchKernelGGL(space_multi_kernel, dim3((uint32_t)((max_rows + 255) / 256), std::min<uint32_t>(65535u, ns - o)), dim3(256), 0, st,
                         (const SpaceJob*)(ds + o));
    HIP_TRY(ctx, hipGetLastError());
  }
  R.ht.fin = host_us_now();
  return ORCGPU_OK;
}

// The dictionary columns' rows and keys, what is left to do behind them, and the summary's way back to the host
int launch_dictionaries_and_post(LaneRun& R) {
  orcgpu_ctx* const ctx = R.ctx;
  int rc = launch_dict_rows(R);
  if (rc) return rc;
  rc = launch_dict_keys(R);
  if (rc) return rc;
  R.ht.dict = host_us_now();
  rc = launch_post_ext(R);
  if (rc) return rc;
  rc = lookup_launch(R);  // (lookup columns: behind the last kernel that writes a column, in front of the computed columns)
  if (rc) return rc;
  rc = computed_launch(R);  // (computed columns: behind the last kernel that writes a column, their counts into the summary)
  if (rc) return rc;
  HIP_TRY(ctx, launch(summary_to_host_kernel, (uint64_t)(R.SL.bytes / 8), false, 256, R.st, (const unsigned long long*)R.dsum, (unsigned long long*)R.hs,
                      (uint64_t)(R.SL.bytes / 8)));
  HIP_TRY(ctx, hipEventRecord(ctx->ev[3], R.st));
  R.ht.enq = host_us_now();
  return ORCGPU_OK;
}

int synchronise(LaneRun& R) {
  HIP_TRY(R.ctx, hipStreamSynchronize(R.st));
  int rc = settle_dict_places(R);
  R.ht.sync = host_us_now();
  return rc;
}

// The GPU's times between the call's events; this lane's launches and the bytes they worked for (orcgpu_last_lane_stats)
void read_timings(LaneRun& R) {
  orcgpu_ctx* const ctx = R.ctx;
  const DecompPlan& DP = R.DP;
  (void)hipEventElapsedTime(&ctx->last_total_ms, ctx->ev[0], ctx->ev[3]);
  (void)hipEventElapsedTime(&ctx->last_expand_ms, ctx->ev[1], ctx->ev[2]);
  static const int edge[6] = {0, 4, 5, 1, 2, 3};  // event index at the start of each phase (+ the end)
  for (int k = 0; k < 5; k++) (void)hipEventElapsedTime(&ctx->last_phase_ms[k], ctx->ev[edge[k]], ctx->ev[edge[k + 1]]);
  (void)hipEventElapsedTime(&ctx->last_phase_ms[5], ctx->ev[0], ctx->ev[6]);
  (void)hipEventElapsedTime(&ctx->last_phase_ms[6], ctx->ev[0], ctx->ev[7]);
  orcgpu_lane_stats& ls = ctx->last_stats;
  ls = orcgpu_lane_stats{};
  ls.lane = (uint32_t)ctx->lane_id;
  ls.n_lanes = 1;
  for (uint32_t si = 0; si < R.n; si++)
    for (size_t ci = 0; ci < R.stripes[si]->cols.size(); ci++) {
      if (R.mask && !(*R.mask)[si][ci]) continue;
      for (auto& sst : R.stripes[si]->streams)
        if (sst.column_id == R.stripes[si]->cols[ci].column_id) ls.stream_bytes += sst.len;
    }
  ls.start_ms = (float)((R.ht.plan - (ctx->call_t0 > 0 ? ctx->call_t0 : R.ht.t0)) * 1e-3);  // (planning done: the launches follow)
  ls.total_ms = ctx->last_total_ms;
  for (int k = 0; k < ORCGPU_N_PHASES; k++) ls.phase_ms[k] = ctx->last_phase_ms[k];
  if (DP.z_lanes && DP.n_zchains && DP.n_chunks) (void)hipEventElapsedTime(&ls.seq_kernel_ms, ctx->ev[9], ctx->ev[8]);
  ls.exec_kernel_ms = ctx->last_phase_ms[0] - ctx->last_phase_ms[5];
  if (ctx->lit_ev_used && hipEventSynchronize(ctx->lit_ev[1]) == hipSuccess) (void)hipEventElapsedTime(&ls.literals_kernel_ms, ctx->lit_ev[0], ctx->lit_ev[1]);
  if (ctx->kev_used[0]) (void)hipEventElapsedTime(&ls.walk_short_kernel_ms, ctx->kev[0][0], ctx->kev[0][1]);
  if (ctx->kev_used[1] && hipEventSynchronize(ctx->kev[1][1]) == hipSuccess) (void)hipEventElapsedTime(&ls.dict_emit_kernel_ms, ctx->kev[1][0], ctx->kev[1][1]);
}

// the exact parallel walk for the lane's next call: when a stream of this one is left damaged by the mending passes
void note_exact_on(LaneRun& R) {
  bool want = false;
  for (int k = 0; k < R.njobs && !want; k++) want = R.hjobs[k].bad_left >= 32u;  // RLE_EXACT_MIN (device/rle_scan.hip)
  R.ctx->exact_on = want;
}

// ORCGPU_DEBUG: the lane's host and GPU times, its jobs, the Zstandard plan, rejected chunks
void debug_report(LaneRun& R) {
  if (!R.host_prof) return;
  orcgpu_ctx* const ctx = R.ctx;
  const Plan& P = R.P;
  const DecompPlan& DP = R.DP;
  const SummaryLayout& SL = R.SL;
  const LaneClock& ht = R.ht;
  uint8_t* const S = R.S;
  uint8_t* const hs = R.hs;
  const RleJob* const hjobs = R.hjobs;
  fprintf(stderr, "[orcgpu] lane %d host us: plan %.1f (columns %.1f, chunk tables %.1f, jobs %.1f)  first launch after %.1f  enqueue %.1f  wait %.1f\n", ctx->lane_id, ht.plan - ht.t0, ht.cols - ht.t0, ht.dp - ht.cols, ht.plan - ht.dp, ht.first - ht.t0, ht.enq - ht.plan, ht.sync - ht.enq);
  fprintf(stderr, "[orcgpu] lane %d enqueue us: decompress %.1f  walk %.1f  present %.1f  expand %.1f  finishers %.1f  dictionary rows %.1f  post %.1f\n", ctx->lane_id,
          ht.first - ht.plan, ht.walk - ht.first, ht.pres - ht.walk, ht.exp - ht.pres, ht.fin - ht.exp, ht.dict - ht.fin, ht.enq - ht.dict);
  fprintf(stderr, "[orcgpu] lane %d GPU ms: decompress %.3f  walk %.3f  present %.3f  expand %.3f  finish %.3f  (total %.3f)\n", ctx->lane_id, ctx->last_phase_ms[0],
          ctx->last_phase_ms[1], ctx->last_phase_ms[2], ctx->last_phase_ms[3], ctx->last_phase_ms[4], ctx->last_total_ms);
  for (int k = 0; k < R.njobs; k++) {
    const JobPlan& j = P.jobs[R.L.order[k]];
    fprintf(stderr, "[orcgpu] job %d (stripe %d col %d role %d block0 %u nbits %d) codec %d blocks %u group %u: bad %u (first %u) repaired %u total %llu\n", k, j.stripe, j.col, j.role, hjobs[k].block0, (int)hjobs[k].nbits, hjobs[k].codec, hjobs[k].nblocks,
            hjobs[k].group_size, hjobs[k].stat_bad, hjobs[k].first_bad, hjobs[k].stat_repaired, (unsigned long long)R.h_scalars()[hjobs[k].total_idx]);
  }
  if (DP.n_zitems) {
    fprintf(stderr, "[orcgpu] zstd plan: %u blocks, %u with sequences (%llu in all): %s\n", DP.n_zblocks, DP.n_zchains, (unsigned long long)DP.z_total_seq,
            DP.z_lanes ? "one lane per block" : "one wavefront per block");
    // the chunks with the most sequences (what the entropy and execution stages last as long as), from the host's copy of the tables
    const ChunkDesc* tc = reinterpret_cast<const ChunkDesc*>(hs + SL.bytes + DP.chunks_off);
    const ZItem* ti = reinterpret_cast<const ZItem*>(hs + SL.bytes + DP.zitems_off);
    std::vector<std::pair<uint64_t, uint32_t>> top;
    for (uint32_t c = 0; c < DP.n_chunks; c++) {
      uint64_t ns = 0;
      for (uint32_t k = tc[c].first_item; k < tc[c].first_item + tc[c].n_items; k++) ns += ti[k].nseq;
      top.push_back({ns, c});
    }
    std::sort(top.rbegin(), top.rend());
    {
      size_t h40 = 0, h20 = 0, h10 = 0, h5 = 0;
      for (auto& t : top) h40 += t.first >= 40000, h20 += t.first >= 20000, h10 += t.first >= 10000, h5 += t.first >= 5000;
      fprintf(stderr, "[orcgpu] zstd chunks: %zu; with >= 40k / 20k / 10k / 5k sequences: %zu / %zu / %zu / %zu\n", top.size(), h40, h20, h10, h5);
    }
    for (size_t k = 0; k < top.size() && k < 6; k++) {
      const uint32_t c = top[k].second, f = tc[c].first_item, e = f + tc[c].n_items;
      uint32_t mxs = 0, lit = 0;
      for (uint32_t q = f; q < e; q++) mxs = std::max(mxs, ti[q].nseq), lit += ti[q].litn;
      fprintf(stderr, "[orcgpu] zstd chunk %u: %u blocks, %llu sequences (largest block %u), %u literal bytes\n", c, e - f, (unsigned long long)top[k].first, mxs, lit);
    }
  }
  if (DP.n_chunks) {
    // diagnostics: where rejected chunks / Zstandard blocks failed
    std::vector<uint8_t> tb(DP.table_bytes);
    (void)hipMemcpy(tb.data(), S + DP.dev_off, DP.table_bytes, hipMemcpyDeviceToHost);
    const ChunkDesc* cc = reinterpret_cast<const ChunkDesc*>(tb.data() + DP.chunks_off);
    const ZBlock* zz = reinterpret_cast<const ZBlock*>(tb.data() + DP.zblocks_off);
    std::vector<uint32_t> zs(2 * DP.n_zblocks + 1);
    if (DP.n_zblocks) (void)hipMemcpy(zs.data(), S + DP.zstatus_off, 8ull * DP.n_zblocks, hipMemcpyDeviceToHost);
    uint32_t shown = 0;
    {
      uint32_t pend = 0, wd = 0;
      for (uint32_t k = 0; k < 2 * DP.n_zblocks; k++) pend += zs[k] == 0xffffffffu, wd += zs[k] == 0x57a7u;
      if (pend || wd) fprintf(stderr, "[orcgpu] entropy jobs: %u of %u still pending, %u watchdog\n", pend, 2 * DP.n_zblocks, wd);
    }
    {
      // DEFLATE: which kernels the call's chunks got (recorded where they were launched), and how many of them the token stage left to the one-wavefront decoder (that
      // decoder does not touch `diag`: the mark is still there) or the execution kernel rejected (its own code in `diag`)
      uint32_t n_deflate = 0, n_deferred = 0, n_exec_bad = 0;
      for (uint32_t k = 0; k < DP.n_chunks; k++)
        if (cc[k].kind == 1) n_deflate++, n_deferred += cc[k].diag == LZX_DEFERRED, n_exec_bad += cc[k].diag != LZX_DEFERRED && cc[k].diag != 0;
      if (n_deflate)
        fprintf(stderr, "[orcgpu] deflate: %u chunks of %u in the call, token stage %u threads per chunk, execution %u threads per chunk, %u deferred to the serial decoder, %u rejected by the execution kernel\n",
                n_deflate, DP.n_chunks, ctx->dbg_inflate_threads, ctx->dbg_exec_threads, n_deferred, n_exec_bad);
    }
    for (uint32_t k = 0; k < DP.n_chunks && shown < 16; k++)
      if (cc[k].status) fprintf(stderr, "[orcgpu] chunk %u (stream %u, kind %u, %u bytes, cap %u): rejected, diag %u\n", k, cc[k].stream, cc[k].kind, cc[k].src_len, cc[k].dst_cap, cc[k].diag), shown++;
    for (uint32_t k = 0; k < DP.n_zblocks && shown < 32; k++)
      if (zs[k] | zs[DP.n_zblocks + k]) fprintf(stderr, "[orcgpu] zstd block %u (chunk %u, nseq %u, lit type %u regen %u): entropy stage code %u\n", k, zz[k].chunk, zz[k].nseq, zz[k].lit_type, zz[k].lit_regen, zs[k] ? zs[k] : zs[DP.n_zblocks + k]), shown++;
  }
#ifdef ORC_PROF
  {
    unsigned long long hp[176];
    hipMemcpyFromSymbol(hp, HIP_SYMBOL(g_prof), sizeof(hp));
    static const struct { int base; const char* who; } sect[] = {{0, "walk"}, {48, "decompress"}, {80, "lz_exec"}, {112, "zstd_entropy"}};
    for (auto& sc : sect)
      for (int k = 0; k < 16; k++)
        if (hp[sc.base + 2 * k]) fprintf(stderr, "[orcgpu] prof %s phase %d: sum %.1f us  max %.2f us\n", sc.who, k, hp[sc.base + 2 * k] * 0.01, hp[sc.base + 2 * k + 1] * 0.01);
    for (int k = 32; k < 48; k++)
      if (hp[k]) fprintf(stderr, "[orcgpu] prof counter %d: %llu\n", k, hp[k]);
    for (int k = 144; k < 176; k++)
      if (hp[k]) fprintf(stderr, "[orcgpu] prof counter %d: %llu\n", k, hp[k]);
    memset(hp, 0, sizeof(hp));
    hipMemcpyToSymbol(HIP_SYMBOL(g_prof), hp, sizeof(hp));
  }
#endif
}

// ---- chunks that need a larger slot ---------------------------------------------------------------------------
// flate2, lzokay and the zstd crate grow their output as needed (compression.rs:142-159, :174-183): a chunk may expand to more
// than the file's compression block size -- no conforming writer emits one, so every chunk gets a slot of the block size,
// and a chunk of those codecs that FAILED in it (whatever the reason: the decoders do not tell an overrun from other damage)
// gets the head-room the oracle gives the crates, max(block size, 4 MiB), and the call is run again.  A chunk that still
// fails is a decoder failure for the reference too.
int grow_failed_slots(LaneRun& R) {
  orcgpu_ctx* const ctx = R.ctx;
  Plan& P = R.P;
  const DecompPlan& DP = R.DP;
  bool codec_error = false;
  const uint64_t* hsc = R.h_scalars();
  for (auto& ds : P.decomp) codec_error = codec_error || hsc[ds.err_idx] != 0;
  if (!codec_error || !DP.n_chunks) return ORCGPU_OK;
  std::vector<ChunkDesc> hc(DP.n_chunks);
  HIP_TRY(ctx, hipMemcpy(hc.data(), R.S + DP.dev_off + DP.chunks_off, (size_t)DP.n_chunks * sizeof(ChunkDesc), hipMemcpyDeviceToHost));
  bool grown = false;
  uint32_t ci = 0;
  for (auto& ds : P.decomp) {
    const int kind = ds.stripe->desc.compression;
    const uint64_t limit = std::max<uint64_t>(ds.stripe->desc.block_size, 1u << 22);
    bool grown_here = false;
    for (auto& c : const_cast<StagedStream*>(ds.st)->chunks) {
      const bool grows = kind == ORCGPU_COMP_ZLIB || kind == ORCGPU_COMP_LZO ||
                         (kind == ORCGPU_COMP_ZSTD && c.zparse >= 0 && !ds.st->zchunks[c.zparse].size_known && !ds.st->zchunks[c.zparse].bad);
      if (!c.original && grows && hc[ci].status && c.plain_cap < limit) {
        c.plain_cap = (uint32_t)limit;
        grown = grown_here = true;
      }
      ci++;
    }
    // (the slots are part of the stream's tables: built again for the second run)
    if (grown_here) build_stream_tables(ds.st->chunks, ds.st->zchunks, kind, ds.st->off, ORC_E_CODEC, const_cast<StagedStream*>(ds.st)->tables);
  }
  return grown ? ORCGPU_RETRY_LARGER_SLOTS : ORCGPU_OK;
}

// ---- resolve errors per column / stripe ----------------------------------------------------------------------
void resolve_column(LaneRun& R, ColPlan& cp) {
  Plan& P = R.P;
  const RleJob* const hjobs = R.hjobs;
  const uint64_t* h_scalars = R.h_scalars();
  const unsigned long long* h_nullc = R.h_nullc();
  if (cp.col < 0) return;  // (an arm of a Union)
  orcgpu_result* r = P.results[cp.stripe];
  ColumnOut& co = r->cols[cp.col];
  for (uint32_t b = 0; b < r->n_batches; b++) co.null_counts[b] = cp.has_present || cp.tz ? h_nullc[cp.nullcount_off + b] : 0;
  // non-null prefix per batch -> map a dense value index to its batch
  auto batch_of_dense = [&](uint64_t d) -> uint32_t {
    uint64_t acc = 0;
    for (uint32_t b = 0; b < r->n_batches; b++) {
      uint64_t rows = std::min<uint64_t>(r->batch, r->n_rows - (uint64_t)b * r->batch);
      acc += rows - co.null_counts[b];
      if (d < acc) return b;
    }
    return r->n_batches ? r->n_batches - 1 : 0;
  };
  int best_status = 0;
  uint32_t best_batch = 0xffffffffu;
  // the stream the error under consideration stems from, and whether the winning error means "stream ran dry"
  const PlainStream* cur_src = nullptr;
  const PlainStream* best_src = nullptr;
  bool best_eof = false;
  auto consider = [&](int code, uint32_t batch) {
    if (code && batch < best_batch) {
      best_batch = batch;
      best_status = code & ~(int)ORC_E_EOF;
      best_eof = (code & (int)ORC_E_EOF) || best_status == (int)ORC_E_IO;
      best_src = cur_src;
    }
  };
  // decode order inside a batch: PRESENT, DATA, LENGTH, SECONDARY, then the finisher
  int jl[4] = {cp.job_present, cp.job_data, cp.job_length, cp.job_secondary};
  // Errors of the same batch: the one the reference meets first wins.  Decimals read the DATA varints
  // before the SECONDARY scales (array_decoder/decimal.rs:131-132), and their DATA errors arrive
  // through the column's own error word.
  unsigned long long fe = h_scalars[cp.err_idx];
  auto consider_fe = [&] {
    if (fe == RLE_NO_ERR) return;
    // Float / Double: the index counts the values the stream holds (dense, i.e. non-null rows): the batch
    // that needs the first missing one fails.  Everything else reports a row.
    const bool dense_index = cp.c.orc_type == ORCGPU_T_FLOAT || cp.c.orc_type == ORCGPU_T_DOUBLE || cp.c.orc_type == ORCGPU_T_UNION;
    cur_src = &cp.data;
    const uint32_t b = dense_index ? batch_of_dense(fe >> 8) : (uint32_t)std::min<uint64_t>(r->n_batches ? r->n_batches - 1 : 0, (fe >> 8) / r->batch);
    consider((int)(fe & 0xff), b);
  };
  const PlainStream* ext_src = cp.is_dict ? &cp.dict : &cp.data;  // dictionary blob / direct values / decimal varints
  const PlainStream* job_src[4] = {&cp.present, &cp.data, &cp.length, &cp.secondary};
  auto consider_job = [&](int k) {
    if (jl[k] < 0) return;
    unsigned long long e = hjobs[P.jobs[jl[k]].final_index].err;
    if (e == RLE_NO_ERR) return;
    uint64_t idx = e >> 8;
    const uint64_t lead = P.jobs[jl[k]].skip_values;  // (values in front of an entry point: a failure there is the first row's)
    idx = idx > lead ? idx - lead : 0;
    int code = (int)(hjobs[P.jobs[jl[k]].final_index].err_pos & 0xff);  // kind: the failure first in the stream (rle_expand.hip: report)
    if (k == 1 && cp.c.orc_type == ORCGPU_T_BOOLEAN) idx *= 8;  // the job counts bytes, the column's dense values are bits
    cur_src = job_src[k];
    consider(code, resolve_job_batch(cp, k, idx, batch_of_dense));
  };
  auto consider_ext = [&] {
    cur_src = ext_src;
    resolve_ext(R, cp, co, r, consider);
  };
  // (k = 0, PRESENT: a decode error there is swallowed like the reference does -- present_words_kernel)
  if (cp.c.orc_type == ORCGPU_T_DECIMAL) {
    consider_ext();  // varint (DATA) errors
    consider_fe();
    for (int k = 1; k < 4; k++) consider_job(k);
  } else if (cp.is_dict) {
    // the dictionary is built when the column's decoder is (string.rs:65-82): its LENGTH stream, then its bytes,
    // fail before any batch does; then per batch the keys (DATA) and their range
    consider_job(2);
    consider_ext();
    consider_job(1);
    consider_fe();
  } else {
    for (int k = 1; k < 4; k++) consider_job(k);
    consider_fe();
    consider_ext();
  }
  // A stream cut short by its container makes the decoder run dry: that failure is reported as the container's
  // own error -- a chunk the block decoder rejected -> Build*Decoder (error.rs), broken chunk framing -> IoError
  // (the reader's sticky status in the oracle; the reference panics in both cases).  Errors met before the
  // cut keep their kind.
  if (best_status && best_eof && best_src && best_src->exists && best_src->err_idx) {
    const uint64_t ce = h_scalars[best_src->err_idx];
    if (ce == ORC_E_CODEC) best_status = ORCGPU_BUILD_DECODER;
    else if (ce == ORC_E_IO) best_status = ORCGPU_IO_ERROR;
  }
  co.status = best_status;
  co.err_batch = best_status ? best_batch : 0;
  // array_decoder/decimal.rs:96-100: every batch of a Decimal column goes through with_precision_and_scale, which is an ArrowError
  // for a precision outside 1 ..= 38, a scale above 38 or above the precision (the reference takes the footer's numbers `as u8` /
  // `as i8`, decimal.rs:59-60): a column of such a type fails at its first batch, behind whatever its streams fail at there.
  if (cp.c.orc_type == ORCGPU_T_DECIMAL && cp.n_rows && r->n_batches) {
    const uint32_t pr = cp.c.precision & 0xffu;
    const int sc = (int8_t)cp.c.scale;
    if ((pr == 0 || pr > 38 || sc > 38 || (sc > 0 && (uint32_t)sc > pr)) && (!co.status || co.err_batch > 0)) {
      co.status = ORCGPU_ARROW;
      co.err_batch = 0;
    }
  }
}

// the lane's host time, part by part (orcgpu_last_lane_host_us)
void note_host_parts(LaneRun& R) {
  orcgpu_ctx* const ctx = R.ctx;
  const LaneClock& t = R.ht;
  if (R.host_prof) fprintf(stderr, "[orcgpu] lane %d host us: post %.1f  (call total %.1f)\n", ctx->lane_id, host_us_now() - t.sync, host_us_now() - t.t0);
  const double parts[ORCGPU_N_HOST_PARTS] = {ctx->call_t0 > 0 ? t.t0 - ctx->call_t0 : 0.0, t.cols - t.t0, t.dp - t.cols, t.plan - t.dp, ctx->hp_fill, ctx->hp_upload + (t.launch - t.plan),
                                             ctx->hp_gate, (t.first - t.launch) - ctx->hp_fill - ctx->hp_upload - ctx->hp_gate, t.enq - t.first, t.sync - t.enq, host_us_now() - t.sync};
  for (int k = 0; k < ORCGPU_N_HOST_PARTS; k++) ctx->last_host_us[k] = (float)parts[k];
}

}  // namespace

// One lane's share of a decode call: the columns `mask` selects (all when null), on the lane's own stream and workspace.
// The results have been created / reset by orcgpu_decode_staged; this fills their selected columns.
static int decode_lane(orcgpu_ctx* ctx, orcgpu_staged* const* stripes, uint32_t n, orcgpu_result** results, const std::vector<std::vector<uint8_t>>* mask) {
  LaneRun R{ctx, ctx->stream, stripes, n, results, mask, getenv("ORCGPU_DEBUG") != nullptr};
  R.ht.t0 = host_us_now();
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = ORCGPU_OK;
  for (auto step : {plan_columns, plan_chunk_tables, lay_out_jobs, reserve_workspace})
    if ((rc = step(R))) return rc;
  fill_summary_mirror(R);
  for (auto step : {launch_decompression, launch_walk, launch_present, launch_expansion, launch_finishers, launch_dictionaries_and_post, synchronise})
    if ((rc = step(R))) return rc;
  read_timings(R);
  note_exact_on(R);
  debug_report(R);
  if ((rc = grow_failed_slots(R))) return rc;
  for (auto& cp : R.P.cols) resolve_column(R, cp);
  lookup_resolve(R);
  computed_resolve(R);
  note_host_parts(R);
  return ORCGPU_OK;
}

static int decode_staged_once(orcgpu_ctx* ctx, orcgpu_staged* const* stripes, uint32_t n, orcgpu_result** results);

// (a second run only when chunks turned out to need larger slots than the compression block size: see grow_failed_slots)
static int decode_staged_retrying(orcgpu_ctx* ctx, orcgpu_staged* const* stripes, uint32_t n, orcgpu_result** results) {
  int rc = decode_staged_once(ctx, stripes, n, results);
  if (rc == ORCGPU_RETRY_LARGER_SLOTS) rc = decode_staged_once(ctx, stripes, n, results);
  return rc == ORCGPU_RETRY_LARGER_SLOTS ? ORCGPU_UNEXPECTED : rc;
}

extern "C" int orcgpu_decode_staged(orcgpu_ctx* ctx, orcgpu_staged* const* stripes, uint32_t n, orcgpu_result** results) {
  if (!ctx || !stripes || !results || !n) return ORCGPU_INVALID_ARGUMENT;
  return decode_staged_retrying(ctx, stripes, n, results);
}

// ---- results: created or reset here, filled column by column by the lanes ------------------------------------------
static int reset_results(orcgpu_ctx* ctx, orcgpu_staged* const* stripes, uint32_t n, orcgpu_result** results) {
  for (uint32_t si = 0; si < n; si++) {
    orcgpu_staged* s = stripes[si];
    if (!s || s->ctx != ctx) return ORCGPU_INVALID_ARGUMENT;
    orcgpu_result* r = results[si];
    if (r && r->hold && orcgpu_hold::hold_exported(r->hold)) {
      set_err(ctx, "a result that exported device batches still view cannot be decoded into again");
      return ORCGPU_INVALID_ARGUMENT;
    }
    // (its exports are released -- on the host: what their consumers enqueued on streams of their own may still read the buffers)
    if (r && r->was_exported) {
      HIP_TRY(ctx, hipDeviceSynchronize());
      r->was_exported = false;
    }
    if (!r) {
      r = new orcgpu_result();
      results[si] = r;
    }
    r->ctx = ctx;
    r->n_rows = s->desc.n_rows;
    r->batch = s->desc.batch_size;
    r->n_batches = (uint32_t)((r->n_rows + r->batch - 1) / r->batch);
    r->words_per_batch = (r->batch + 63) / 64;
    r->cols.assign(s->cols.size(), ColumnOut{});
    for (size_t ci = 0; ci < s->cols.size(); ci++) {
      ColumnOut& co = r->cols[ci];
      co.column_id = s->cols[ci].column_id;
      co.orc_type = s->cols[ci].orc_type;
      const uint32_t par = s->cols[ci].parent;
      if (par && par <= ci) {
        co.parent = (int32_t)par - 1;
        const int pt = s->cols[par - 1].orc_type;
        co.elem = r->cols[par - 1].elem || pt == ORCGPU_T_LIST || pt == ORCGPU_T_MAP;
      }
    }
    for (auto* sub : r->subs) orcgpu_result_free(sub);
    r->subs.clear();
    lookup_append_columns(s, r);
    computed_append_columns(s, r);
    r->status = 0;
    r->err_batch = r->err_col = 0;
    if (r->mirror) r->mirror->wait();  // (a copy of the previous contents still on its way to the host reads these buffers)
    r->mirror_valid = false;
    r->dev_ready_recorded = false;
    r->selected = false;
    r->sel.clear();
    r->filtered = false;
    r->filt_used = 0;
    for (int l = 0; l < kMaxLanes; l++) r->arena_used[l] = r->chars_used[l] = 0;
  }
  return ORCGPU_OK;
}

// ---- lanes: whole columns, balanced by their staged bytes (longest first); a column that alone is a quarter of the
// call gets a lane to itself (its decompression is a serial chain per block: what runs beside it is free) -------------
// ORCGPU_LANES = 1..4 forces the count.  Unset: two lanes for calls that are big enough and whose Zstandard blocks differ enough
// for the heavy / light split below to pay (lineitem SF1: 10.9 -> 10.1 ms); otherwise one -- lanes with equally long
// decompression phases have nothing to overlap, and every extra stream slows the short kernels of the others.
// Returns the number of lanes and, for more than one, the columns of each per stripe (`masks`) and the call's Zstandard path.
static int choose_lanes(orcgpu_staged* const* stripes, uint32_t n, std::vector<std::vector<std::vector<uint8_t>>>& masks, int& call_z) {
  const int forced_lanes = [] {  // (read at every call: the tests run the same stripes through every lane count)
    const char* e = getenv("ORCGPU_LANES");
    int v = e ? atoi(e) : 0;
    return v < 0 ? 0 : (v > kMaxLanes ? kMaxLanes : v);
  }();
  size_t max_cols = 0;
  for (uint32_t si = 0; si < n; si++) max_cols = std::max(max_cols, stripes[si]->cols.size());
  int want_lanes = forced_lanes ? forced_lanes : 1;
  if (!forced_lanes && max_cols >= 4) {
    uint64_t staged = 0;
    uint32_t mx_all = 0;
    for (uint32_t si = 0; si < n; si++)
      for (auto& st : stripes[si]->streams) {
        staged += st.len;
        mx_all = std::max(mx_all, st.tables.max_nseq);
      }
    if (staged >= (64ull << 20) && mx_all >= 16384) want_lanes = 2;
  }
  for (uint32_t si = 0; si < n; si++)
    if (stripes[si]->computed || stripes[si]->lookup) want_lanes = 1;  // (computed columns: the operands complete on the stream that evaluates)
  int n_lanes = (int)std::min<size_t>((size_t)want_lanes, max_cols);
  if (n_lanes <= 1) return n_lanes;
  // the weight of a root column = staged bytes of the streams of its columns over all stripes of the call; one pass per stripe,
  // through the stripe's columns by id (the first of that id counts, as many times as the id is given) and their roots
  std::vector<LaneRoot> roots;
  std::map<uint32_t, uint32_t> root_at;                   // root column id -> index in `roots`
  std::vector<std::vector<uint32_t>> root_of(n);          // [stripe][column] -> index in `roots`
  std::vector<std::pair<uint32_t, uint32_t>> stray;       // (column id, longest block) of streams of no column of their stripe
  uint64_t seq_all = 0;
  for (uint32_t si = 0; si < n; si++) {
    const auto& cols = stripes[si]->cols;
    std::map<uint32_t, std::pair<uint32_t, uint32_t>> by_id;  // column id -> (first column of that id, columns of that id)
    for (size_t ci = 0; ci < cols.size(); ci++) by_id.insert({cols[ci].column_id, {(uint32_t)ci, 0u}}).first->second.second++;
    root_of[si].resize(cols.size());
    for (size_t ci = 0; ci < cols.size(); ci++) {
      size_t k = by_id[cols[ci].column_id].first;
      while (cols[k].parent && cols[k].parent <= k) k = cols[k].parent - 1;
      const auto at = root_at.insert({cols[k].column_id, (uint32_t)roots.size()});
      if (at.second) roots.push_back(LaneRoot{cols[k].column_id, 0, 0});
      root_of[si][ci] = at.first->second;
    }
    for (auto& st : stripes[si]->streams) {
      seq_all += st.tables.total_seq;
      const auto c = by_id.find(st.column_id);
      if (c == by_id.end()) {
        stray.push_back({st.column_id, st.tables.max_nseq});
        continue;
      }
      LaneRoot& root = roots[root_of[si][c->second.first]];
      root.bytes += st.len * c->second.second;
      root.max_nseq = std::max(root.max_nseq, st.tables.max_nseq);
    }
  }
  for (auto& s : stray) {
    const auto at = root_at.find(s.first);
    if (at != root_at.end()) roots[at->second].max_nseq = std::max(roots[at->second].max_nseq, s.second);
  }
  const LaneDeal D = deal_lanes(roots, seq_all, n_lanes, forced_lanes != 0);
  call_z = D.call_z;
  masks.assign(D.n_lanes, {});
  for (int l = 0; l < D.n_lanes; l++) {
    masks[l].resize(n);
    for (uint32_t si = 0; si < n; si++) {
      masks[l][si].resize(root_of[si].size());
      for (size_t ci = 0; ci < root_of[si].size(); ci++) masks[l][si][ci] = D.lane_of[root_of[si][ci]] == l;
    }
  }
  return D.n_lanes;
}

// The lanes beside the caller's own are opened when first needed; every lane decodes its columns on a thread of its own
static int run_lanes(orcgpu_ctx* ctx, orcgpu_staged* const* stripes, uint32_t n, orcgpu_result** results, const std::vector<std::vector<std::vector<uint8_t>>>& masks, int n_lanes) {
  if (n_lanes <= 1) return decode_lane(ctx, stripes, n, results, nullptr);
  int rc = ORCGPU_OK;
  const double call_t0 = ctx->call_t0;
  for (int l = 1; l < n_lanes; l++)
    if (!ctx->lanes[l]) {
      orcgpu_ctx* c = open_ctx(ctx->device, nullptr, l);
      if (!c) {
        set_err(ctx, "could not create lane %d", l);
        return ORCGPU_HIP_ERROR;
      }
      c->lane_id = l;
      ctx->lanes[l] = c;
    }
  for (int l = 1; l < n_lanes; l++) ctx->lanes[l]->call_t0 = call_t0;
  for (int l = 1; l < n_lanes; l++) ctx->lanes[l]->call_z_lanes = ctx->call_z_lanes;
  for (int l = 0; l < n_lanes; l++) {
    orcgpu_ctx* c = ctx->lanes[l];
    c->tables_gate.store(0);
    c->n_gate_peers = 0;
    for (int o = 0; o < n_lanes; o++)
      if (o != l) c->gate_peers[c->n_gate_peers++] = ctx->lanes[o];
  }
  std::vector<int> rcs(n_lanes, 0);
  std::vector<std::thread> th;
  for (int l = 1; l < n_lanes; l++) th.emplace_back([&, l] { rcs[l] = decode_lane(ctx->lanes[l], stripes, n, results, &masks[l]); });
  rcs[0] = decode_lane(ctx, stripes, n, results, &masks[0]);
  for (auto& t : th) t.join();
  int slow = 0;
  for (int l = 0; l < n_lanes; l++) {
    if (rcs[l] && !rc) {
      rc = rcs[l];
      if (l) ctx->err = ctx->lanes[l]->err;
    }
    if (ctx->lanes[l]->last_total_ms > ctx->lanes[slow]->last_total_ms) slow = l;
  }
  if (slow) {  // timing hooks report the lane that took longest
    orcgpu_ctx* c = ctx->lanes[slow];
    ctx->last_total_ms = c->last_total_ms;
    ctx->last_expand_ms = c->last_expand_ms;
    ctx->last_expand_launches = c->last_expand_launches;
    for (int k = 0; k < ORCGPU_N_PHASES; k++) ctx->last_phase_ms[k] = c->last_phase_ms[k];
  }
  return rc;
}

// The stripes' status (the failing column of the earliest failing batch) and the Arrow bytes decoded, per result and per lane
static void sum_up_results(orcgpu_ctx* ctx, uint32_t n, orcgpu_result** results, int n_lanes) {
  ctx->last_n_lanes = (uint32_t)std::max(1, n_lanes);
  for (int l = 0; l < std::max(1, n_lanes); l++) {
    ctx->lanes[l]->last_stats.n_lanes = ctx->last_n_lanes;
    ctx->lanes[l]->last_stats.arrow_bytes = 0;
  }
  for (uint32_t si = 0; si < n; si++) {
    orcgpu_result* r = results[si];
    r->status = 0;
    uint32_t bb = 0xffffffffu;
    r->arrow_bytes = 0;
    for (size_t ci = 0; ci < r->cols.size(); ci++) {
      ColumnOut& co = r->cols[ci];
      if (co.status && co.err_batch < bb) {
        bb = co.err_batch;
        r->status = co.status;
        r->err_batch = co.err_batch;
        r->err_col = (uint32_t)ci;
      }
      if (!co.elem) {
        const uint64_t cb = result_column_bytes(r, co);
        r->arrow_bytes += cb;
        if (co.lane >= 0 && co.lane < std::max(1, n_lanes)) ctx->lanes[co.lane]->last_stats.arrow_bytes += cb;
      }
    }
  }
}

// The virtual stripe of the elements of List / Map column `ci`, `total` of them: its rows are the elements, ONE batch; its root
// columns the element column (a Map: key and value) with everything below; its streams those of the staged stripe.
static std::unique_ptr<orcgpu_staged> element_stripe(const orcgpu_staged* s, const orcgpu_result* r, size_t ci, uint64_t total, std::vector<uint32_t>& src) {
  auto v = std::make_unique<orcgpu_staged>();
  v->ctx = s->ctx;
  v->desc = s->desc;
  v->desc.n_rows = total;
  v->desc.batch_size = (uint32_t)std::max<uint64_t>(total, 1);
  v->dev = s->dev;
  v->dev_bytes = s->dev_bytes;
  v->zone = s->zone;
  v->ready = nullptr;  // (the stripe's bytes have arrived: its own decode has just run)
  // the subtree below column ci, parents re-numbered (the direct children become root columns)
  std::vector<uint32_t> map_new(s->cols.size(), 0);  // 1 + new index
  for (size_t k = ci + 1; k < s->cols.size(); k++) {
    const uint32_t par = s->cols[k].parent;
    if (!par || par > k) continue;
    const bool child = par - 1 == ci, below = map_new[par - 1] != 0;
    if (!child && !below) continue;
    orcgpu_column c = s->cols[k];
    c.parent = child ? 0u : map_new[par - 1];
    v->cols.push_back(c);
    // (the column of the caller's stripe this one stands for: `s` is itself a virtual stripe when the List lies inside a List)
    src.push_back(r->src_col.empty() ? (uint32_t)k : r->src_col[k]);
    map_new[k] = (uint32_t)v->cols.size();
  }
  for (auto& st : s->streams)
    for (auto& c : v->cols)
      if (c.column_id == st.column_id) {
        v->streams.push_back(st);
        v->stream_bytes += st.len;
        break;
      }
  return v;
}

// ---- the elements of List / Map columns (list.rs:63-87, map.rs:74-104: `inner.next_batch(total_length, None)`) -----------
// Their count is known now.  Per such column a "stripe" of its own (element_stripe).  All of
// them go through one more decode call together, which takes care of Lists inside them the same way.
static int decode_list_elements(orcgpu_ctx* ctx, orcgpu_staged* const* stripes, uint32_t n, orcgpu_result** results) {
  std::vector<std::unique_ptr<orcgpu_staged>> vst;
  std::vector<orcgpu_staged*> vptr;
  std::vector<orcgpu_result*> vres;
  struct Owner {
    uint32_t si, col;
  };
  std::vector<Owner> owner;
  for (uint32_t si = 0; si < n; si++) {
    orcgpu_staged* s = stripes[si];
    orcgpu_result* r = results[si];
    for (size_t ci = 0; ci < r->cols.size(); ci++) {
      ColumnOut& co = r->cols[ci];
      if (!co.is_list || co.elem) continue;
      uint64_t total = 0;
      for (auto v : co.char_total) total += v;
      if (total >= (1ull << 31)) {
        set_err(ctx, "column %u: %llu elements in one stripe: more than 2^31 - 1 are not supported", co.column_id, (unsigned long long)total);
        return ORCGPU_INVALID_ARGUMENT;
      }
      std::vector<uint32_t> src;
      auto v = element_stripe(s, r, ci, total, src);
      orcgpu_result* sub = new orcgpu_result();
      sub->src_col = src;
      co.sub = (int32_t)r->subs.size();
      r->subs.push_back(sub);
      vptr.push_back(v.get());
      vres.push_back(sub);
      vst.push_back(std::move(v));
      owner.push_back(Owner{si, (uint32_t)ci});
    }
  }
  if (vptr.empty()) return ORCGPU_OK;
  const int rc2 = decode_staged_retrying(ctx, vptr.data(), (uint32_t)vptr.size(), vres.data());
  for (auto& v : vst) v->dev = nullptr;  // (borrowed)
  if (rc2) return rc2;
  for (size_t k = 0; k < vres.size(); k++) {
    orcgpu_result* r = results[owner[k].si];
    r->arrow_bytes += vres[k]->arrow_bytes;
    // a failure among the elements: its place among the rows is not kept (the elements are one batch) -- the stripe fails in
    // its first batch, unless an earlier column already fails there
    if (vres[k]->status && !r->status) {
      r->status = vres[k]->status;
      r->err_batch = 0;
      r->err_col = owner[k].col;
    }
    // map.rs:90-99: the keys and the values of a Map become a StructArray whose `keys` field is not nullable -- a key column with a
    // null in it (a file that holds a PRESENT stream for the keys, or one whose bytes were damaged) is an ArrowError there
    // ("Found unmasked nulls for non-nullable StructArray field"), and an array no Arrow implementation imports here (Arrow C++
    // aborts the process on it).  Like every failure among the elements it is the stripe's first batch that fails.
    if (!r->status && r->cols[owner[k].col].orc_type == ORCGPU_T_MAP && !vres[k]->cols.empty()) {
      uint64_t key_nulls = 0;
      for (uint64_t c : vres[k]->cols[0].null_counts) key_nulls += c;
      if (key_nulls) {
        r->status = ORCGPU_ARROW;
        r->err_batch = 0;
        r->err_col = owner[k].col;
      }
    }
  }
  return ORCGPU_OK;
}

static int decode_staged_once(orcgpu_ctx* ctx, orcgpu_staged* const* stripes, uint32_t n, orcgpu_result** results) {
  const double call_t0 = host_us_now();
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  int rc = reset_results(ctx, stripes, n, results);
  if (rc) return rc;
  std::vector<std::vector<std::vector<uint8_t>>> masks;
  int call_z = -1;  // the call's Zstandard path, decided when the call is split over lanes
  const int n_lanes = choose_lanes(stripes, n, masks, call_z);
  ctx->call_t0 = call_t0;
  ctx->call_z_lanes = n_lanes > 1 ? call_z : -1;
  ctx->n_gate_peers = 0;
  ctx->tables_gate.store(0);
  const double t_pre = host_us_now();
  rc = run_lanes(ctx, stripes, n, results, masks, n_lanes);
  const double t_lanes = host_us_now();
  if (getenv("ORCGPU_DEBUG")) fprintf(stderr, "[orcgpu] call host us: before the lanes %.1f, lanes %.1f\n", t_pre - call_t0, t_lanes - t_pre);
  if (rc) return rc;
  sum_up_results(ctx, n, results, n_lanes);
  rc = decode_list_elements(ctx, stripes, n, results);
  if (rc) return rc;
  if (getenv("ORCGPU_DEBUG")) fprintf(stderr, "[orcgpu] call host us: behind the lanes %.1f\n", host_us_now() - t_lanes);
  return ORCGPU_OK;
}

extern "C" int orcgpu_stripe_decode(orcgpu_ctx* ctx, const orcgpu_stripe_desc* desc, orcgpu_result** out) {
  if (!out) return ORCGPU_INVALID_ARGUMENT;
  orcgpu_staged* s = nullptr;
  int rc = orcgpu_stage_stripe(ctx, desc, &s);
  if (rc) return rc;
  orcgpu_result* r = nullptr;
  rc = orcgpu_decode_staged(ctx, &s, 1, &r);
  orcgpu_staged_free(s);
  if (rc) {
    orcgpu_result_free(r);
    return rc;
  }
  *out = r;
  return ORCGPU_OK;
}

extern "C" int orcgpu_last_phase_ms(const orcgpu_ctx* ctx, float* ms, uint32_t n) {
  if (!ctx || !ms) return ORCGPU_INVALID_ARGUMENT;
  for (uint32_t k = 0; k < n && k < ORCGPU_N_PHASES; k++) ms[k] = ctx->last_phase_ms[k];
  return ORCGPU_OK;
}

extern "C" int orcgpu_last_lane_stats(const orcgpu_ctx* ctx, uint32_t lane, orcgpu_lane_stats* out) {
  if (!ctx || !out || lane >= ctx->last_n_lanes || lane >= (uint32_t)kMaxLanes || !ctx->lanes[lane]) return ORCGPU_INVALID_ARGUMENT;
  *out = ctx->lanes[lane]->last_stats;
  return ORCGPU_OK;
}

extern "C" int orcgpu_last_lane_host_us(const orcgpu_ctx* ctx, uint32_t lane, float* us, uint32_t n) {
  if (!ctx || !us || lane >= ctx->last_n_lanes || lane >= (uint32_t)kMaxLanes || !ctx->lanes[lane]) return ORCGPU_INVALID_ARGUMENT;
  for (uint32_t k = 0; k < n && k < ORCGPU_N_HOST_PARTS; k++) us[k] = ctx->lanes[lane]->last_host_us[k];
  return ORCGPU_OK;
}

extern "C" int orcgpu_last_timing(const orcgpu_ctx* ctx, float* total_ms, float* expand_ms, uint32_t* expand_launches) {
  if (!ctx) return ORCGPU_INVALID_ARGUMENT;
  if (total_ms) *total_ms = ctx->last_total_ms;
  if (expand_ms) *expand_ms = ctx->last_expand_ms;
  if (expand_launches) *expand_launches = ctx->last_expand_launches;
  return ORCGPU_OK;
}
