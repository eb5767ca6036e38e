// orcgpu_lookup.inc -- lookup columns inside the decode call (include/orcgpu.h: "Key maps and lookup columns"; the plan:
// orcgpu_lookup_plan.inc; the kernel: device/key_map_kernels.hip: lookup_columns_kernel).  Included by orcgpu_decode.inc behind
// LaneRun, in front of orcgpu_computed.inc, which it mirrors step for step.
//
// A staged stripe that carries a plan (orcgpu_staged::lookup, set by the file reader) gets its lookup columns as ordinary ColumnOut
// records behind the file's columns and in front of the computed ones:
//   reset_results      appends the records (lookup_append_columns): type, width, precision, scale -- what the map's seal fixed
//   choose_lanes       keeps such a call on ONE lane: the probe keys must be complete on the stream that probes
//   plan_columns       reserves values and validity in the lane's result arena, the null counts in the call's summary, one
//                      LookupJob per (map, key column) pair in the workspace (lookup_plan_stripe)
//   launch_dictionaries_and_post   uploads the jobs and launches lookup_columns_kernel behind the last kernel that writes a column,
//                      in front of compute_columns_kernel and the summary's copy (lookup_launch): no wait of its own
//   decode_lane        reads the counts out of the summary with everything else (lookup_resolve)
// The result arena owns the columns' buffers, like every column's.  The MAP's memory is the plan's: every LookupPair holds a share
// (LookupMapRef::hold), the plan travels with the reader and with every staged stripe, so the handle may be freed under a live
// reader -- hipFree waits for the device, so a kernel that still probes has run when the memory goes.
// A stripe whose decode failed is still probed -- nobody knows of the failure before the closing wait --: every index is masked or
// clamped, the batches in front of the failing one are good, the others are never handed out.
// A reader without lookup columns: orcgpu_staged::lookup is null, every function here returns at its first line, nothing is
// appended, reserved, uploaded or launched.

namespace {

void lookup_append_columns(const orcgpu_staged* s, orcgpu_result* r) {
  if (!s->lookup) return;
  for (const orcgpu_host::LookupColumn& c : s->lookup->cols) {
    ColumnOut co{};
    co.computed = true;  // (no column of the file: its field is nullable whatever the batch holds)
    co.orc_type = orcgpu_host::lookup_orc_type(c.v);
    co.column_id = 0;
    co.width = key_map_value_width(c.v.kind);
    co.precision = c.v.kind == KMV_DEC128 ? c.v.precision : 0;
    co.scale = c.v.kind == KMV_DEC128 ? c.v.scale : 0;
    co.has_present = true;
    r->cols.push_back(co);
  }
}

// the probe key as the decode laid it out: a flat integer column
bool lookup_key_fits(const ColumnOut& oc) {
  if (oc.is_string || oc.is_bool || oc.dict_out || oc.is_struct || oc.is_union || oc.is_list || oc.elem || oc.parent >= 0 || oc.computed) return false;
  const bool is_int = oc.orc_type == ORCGPU_T_BYTE || oc.orc_type == ORCGPU_T_SHORT || oc.orc_type == ORCGPU_T_INT || oc.orc_type == ORCGPU_T_LONG || oc.orc_type == ORCGPU_T_DATE;
  return is_int && (oc.width == 1 || oc.width == 2 || oc.width == 4 || oc.width == 8);
}
int lookup_check_keys(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_host::LookupPlan& plan, size_t n_file) {
  for (const orcgpu_host::LookupPair& p : plan.pairs)
    if (p.key_col >= n_file || !lookup_key_fits(r->cols[p.key_col])) {
      set_err(ctx, "lookup columns: column %u of the stripe is not decoded to the integers a probe key is taken as", p.key_col < n_file ? r->cols[p.key_col].column_id : p.key_col);
      return ORCGPU_MISMATCHED_SCHEMA;
    }
  return ORCGPU_OK;
}

// values and validity of the lookup columns r->cols[first .. first + n) in the arena of `lane`
void lookup_place_columns(orcgpu_result* r, size_t first, size_t n, int lane, Bump& RB) {
  for (size_t k = first; k < first + n; k++) {
    ColumnOut& co = r->cols[k];
    co.lane = lane;
    co.values_bytes = r->n_rows * co.width;
    co.values_off = RB.take(co.values_bytes + 16);
    co.validity_off = RB.take((uint64_t)r->n_batches * r->words_per_batch * 8 + 16);
    co.null_counts.assign(r->n_batches, 0);
    co.status = 0;
  }
}

uint64_t lookup_table_bytes(const orcgpu_host::LookupPlan& plan) { return plan.pairs.size() * sizeof(LookupJob) + 16; }

// The jobs filled and uploaded to T, the kernel enqueued on `st`.  d_counts: n columns x n_batches null counts, zero.
int lookup_enqueue(orcgpu_ctx* ctx, hipStream_t st, orcgpu_result* r, const orcgpu_host::LookupPlan& plan, size_t n_file, uint8_t* T, unsigned long long* d_counts) {
  std::vector<LookupJob> jobs(plan.pairs.size());
  for (size_t p = 0; p < plan.pairs.size(); p++) {
    const orcgpu_host::LookupPair& pr = plan.pairs[p];
    const orcgpu_host::LookupMapRef& m = pr.map;
    LookupJob& j = jobs[p];
    memset(&j, 0, sizeof(j));
    const ColumnOut& kc = r->cols[pr.key_col];
    const uint8_t* KA = r->arena[kc.lane].p;
    j.key.validity = kc.has_present ? reinterpret_cast<const unsigned long long*>(KA + kc.validity_off) : nullptr;
    j.key.values = KA + kc.values_off;
    j.key.width = kc.width;
    j.key.kind = FKIND_INT;
    j.table = reinterpret_cast<const uint8_t*>((uintptr_t)m.table);
    j.table_bytes = m.table_bytes;
    j.n_slots = m.n_slots;
    j.n_values = (uint32_t)std::min<size_t>(pr.cols.size(), kKeyMapMaxValues);
    for (uint32_t k = 0; k < j.n_values; k++) {
      const orcgpu_host::LookupColumn& c = plan.cols[pr.cols[k]];
      const ColumnOut& co = r->cols[n_file + pr.cols[k]];
      uint8_t* const A = r->arena[co.lane].p;
      const uint8_t* const planes = reinterpret_cast<const uint8_t*>((uintptr_t)m.planes);
      j.v[k].plane = planes + m.lay.o_values[c.value];
      j.v[k].valid = planes + m.lay.o_valid[c.value];
      j.v[k].out_values = A + co.values_off;
      j.v[k].out_validity = reinterpret_cast<unsigned long long*>(A + co.validity_off);
      j.v[k].null_counts = d_counts + (uint64_t)pr.cols[k] * r->n_batches;
      j.v[k].width = co.width;
    }
  }
  HIP_TRY(ctx, ctx->upload(T, jobs.data(), jobs.size() * sizeof(LookupJob), st));
  const uint64_t n_words = (uint64_t)r->n_batches * r->words_per_batch;
  hipLaunchKernelGGL(lookup_columns_kernel, dim3((uint32_t)((n_words + 3) / 4), (uint32_t)jobs.size()), dim3(256), 0, st, reinterpret_cast<const LookupJob*>(T), r->n_rows,
                     r->n_batches, r->batch, r->words_per_batch);
  HIP_TRY(ctx, hipGetLastError());
  return ORCGPU_OK;
}

int lookup_plan_stripe(LaneRun& R, uint32_t si) {
  orcgpu_staged* s = R.stripes[si];
  if (!s->lookup) return ORCGPU_OK;
  orcgpu_result* r = R.results[si];
  Plan& P = R.P;
  const orcgpu_host::LookupPlan& plan = *s->lookup;
  const size_t n_file = s->cols.size(), n = plan.cols.size();
  if (R.mask || r->cols.size() < n_file + n) {
    set_err(R.ctx, "lookup columns: the decode call is not laid out for them");
    return ORCGPU_UNEXPECTED;
  }
  if (const int rc = lookup_check_keys(R.ctx, r, plan, n_file)) return rc;
  LaneRun::LookupPlace place;
  place.stripe = si;
  place.first_col = (uint32_t)n_file;
  place.n_cols = (uint32_t)n;
  place.nullcount_off = (uint32_t)P.n_nullcount_slots;
  P.n_nullcount_slots += (uint64_t)n * r->n_batches;
  lookup_place_columns(r, n_file, n, P.lane_id, P.result_bump[si]);
  place.table_off = P.scratch.take(lookup_table_bytes(plan));
  R.lookup.push_back(place);
  return ORCGPU_OK;
}

int lookup_launch(LaneRun& R) {
  for (const LaneRun::LookupPlace& place : R.lookup) {
    orcgpu_staged* s = R.stripes[place.stripe];
    orcgpu_result* r = R.results[place.stripe];
    if (!r->n_rows || !r->n_batches) continue;
    if (const int rc = lookup_enqueue(R.ctx, R.st, r, *s->lookup, place.first_col, R.S + place.table_off, R.d_nullc + place.nullcount_off)) return rc;
  }
  return ORCGPU_OK;
}

void lookup_resolve(LaneRun& R) {
  const unsigned long long* h_nullc = R.h_nullc();
  for (const LaneRun::LookupPlace& place : R.lookup) {
    orcgpu_result* r = R.results[place.stripe];
    for (size_t k = 0; k < place.n_cols; k++) {
      ColumnOut& co = r->cols[place.first_col + k];
      for (uint32_t b = 0; b < r->n_batches; b++) co.null_counts[b] = h_nullc[place.nullcount_off + k * r->n_batches + b];
    }
  }
}

// The same on a decoded result, for a caller that decoded by hand: the columns appended behind the result's own, in lane 0's arena
// (grown, its contents kept, when the decode left no room behind them), probed on the decode stream; ONE wait of its own brings
// the null counts back.  Before any row selection, row filter or computed column on the result; a failed result is left alone.
int result_lookup_columns(orcgpu_ctx* ctx, orcgpu_result* r, const orcgpu_host::LookupPlan& plan) {
  if ((r->hold && orcgpu_hold::hold_exported(r->hold)) || r->selected || r->filtered) {
    set_err(ctx, "lookup columns: the result has been selected on, filtered or exported: look its columns up first");
    return ORCGPU_INVALID_ARGUMENT;
  }
  const size_t n_file = r->cols.size(), n = plan.cols.size();
  if (const int rc = lookup_check_keys(ctx, r, plan, n_file)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  orcgpu_staged shape;  // (what lookup_append_columns reads of a staged stripe: the plan)
  shape.lookup = std::make_shared<const orcgpu_host::LookupPlan>(plan);
  lookup_append_columns(&shape, r);
  Bump RB;
  RB.off = r->arena_used[0];
  lookup_place_columns(r, n_file, n, 0, RB);
  const uint64_t need = RB.off;
  DevBuf old;
  if (need + kAlign > r->arena[0].cap) {  // grow lane 0's arena: a new one, the decode's bytes copied over
    DevBuf grown;
    if (!grown.ensure(need + kAlign)) {
      r->cols.resize(n_file);
      set_err(ctx, "hipMalloc(%llu) for the lookup columns failed", (unsigned long long)need);
      return ORCGPU_HIP_ERROR;
    }
    if (r->arena_used[0]) HIP_TRY(ctx, hipMemcpyAsync(grown.p, r->arena[0].p, r->arena_used[0], hipMemcpyDeviceToDevice, st));
    old = r->arena[0];
    r->arena[0] = grown;
  }
  r->arena_used[0] = need;
  const size_t n_counts = (size_t)n * r->n_batches;
  std::vector<unsigned long long> back(n_counts + 1, 0);
  int rc = ORCGPU_OK;
  if (r->n_rows && r->n_batches) {
    const uint64_t o_counts = align_up(lookup_table_bytes(plan), 16);
    if (!r->filt_tmp.ensure(o_counts + n_counts * 8 + kAlign)) {
      set_err(ctx, "hipMalloc for the lookup columns' tables failed");
      rc = ORCGPU_HIP_ERROR;
    }
    uint8_t* T = r->filt_tmp.p;
    unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(T + o_counts);
    if (!rc && hipMemsetAsync(d_counts, 0, n_counts * 8, st) != hipSuccess) rc = ORCGPU_HIP_ERROR;
    if (!rc) rc = lookup_enqueue(ctx, st, r, plan, n_file, T, d_counts);
    if (!rc && hipMemcpyAsync(back.data(), d_counts, n_counts * 8, hipMemcpyDeviceToHost, st) != hipSuccess) rc = ORCGPU_HIP_ERROR;
  }
  // ---- the call's one wait: the null counts ----
  if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = ORCGPU_HIP_ERROR;
  old.release();
  if (rc) {
    if (rc == ORCGPU_HIP_ERROR) set_err(ctx, "lookup columns: a HIP call failed");
    r->cols.resize(n_file);
    return rc;
  }
  for (size_t k = 0; k < n; k++) {
    ColumnOut& co = r->cols[n_file + k];
    for (uint32_t b = 0; b < r->n_batches; b++) co.null_counts[b] = back[k * r->n_batches + b];
    r->arrow_bytes += result_column_bytes(r, co);
  }
  r->mirror_valid = false;
  r->dev_ready_recorded = false;
  return ORCGPU_OK;
}

}  // namespace
