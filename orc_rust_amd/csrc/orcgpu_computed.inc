// orcgpu_computed.inc -- computed columns inside the decode call (include/orcgpu.h: "Computed columns"; the plan:
// orcgpu_computed_plan.inc; the kernel: device/compute_kernels.hip).  Included by orcgpu_decode.inc behind LaneRun.
//
// A staged stripe that carries a plan (orcgpu_staged::computed, set by the file reader) gets its computed columns as ordinary
// ColumnOut records behind the file's columns:
//   reset_results      appends the records (computed_append_columns): type, width, scale -- what the plan fixed
//   choose_lanes       keeps such a call on ONE lane: the operands must be complete on the stream that evaluates
//   plan_columns       reserves values and validity in the lane's result arena, the null counts (and one overflow count a stripe)
//                      in the call's summary, the kernel's tables in the workspace (computed_plan_stripe)
//   launch_dictionaries_and_post   uploads the tables and launches compute_columns_kernel behind the last kernel that writes a
//                      column, in front of the summary's copy (computed_launch): no wait of its own
//   decode_lane        reads the counts out of the summary with everything else (computed_resolve)
// The reader's row selection on a stripe's rows is fixed when the stripe is staged (orcgpu_staged::sel), before the decode call:
// every row gets its value, the overflow COUNT is of the selected rows (the kernel searches the selection's batches for an
// overflowed row).  orcgpu_result_compute_columns is the same on a hand-decoded result, with one wait of its own.
// The result arena owns the buffers, like every column's: they are reused, copied back, selected from, gathered from and exported
// by the code that serves the file's columns.  A stripe whose decode failed still has the columns evaluated -- nobody knows of the
// failure before the closing wait --: the batches in front of the failing one are good, the others are never handed out.
// A reader without computed columns: orcgpu_staged::computed is null, every function here returns at its first line, nothing is
// appended, reserved, uploaded or launched.

namespace {

void computed_append_columns(const orcgpu_staged* s, orcgpu_result* r) {
  r->computed_overflow = 0;
  if (!s->computed) return;
  for (const orcgpu_host::ComputedColumn& c : s->computed->cols) {
    ColumnOut co{};
    co.computed = true;
    co.orc_type = orcgpu_host::computed_orc_type(c);
    co.column_id = 0;  // (no column of the file)
    co.width = orcgpu_host::computed_width(c);
    co.precision = c.cls == orcgpu_host::XCLASS_DEC ? 38 : 0;
    co.scale = c.cls == orcgpu_host::XCLASS_DEC ? (uint32_t)c.scale : 0;
    co.has_present = true;
    r->cols.push_back(co);
  }
}

// the operand as the decode lays it out against what the program loads from it
bool computed_operand_fits(const ColumnOut& oc, uint32_t push_op) {
  if (oc.is_string || oc.is_bool || oc.dict_out || oc.is_struct || oc.is_union || oc.is_list || oc.elem || oc.parent >= 0 || oc.computed) return false;
  const bool is_float = oc.orc_type == ORCGPU_T_FLOAT || oc.orc_type == ORCGPU_T_DOUBLE;
  if (push_op == AX_PUSH_F64) return is_float && (oc.width == 4 || oc.width == 8);
  if (push_op == AX_PUSH_DEC) return oc.orc_type == ORCGPU_T_DECIMAL && oc.width == 16;
  const bool is_int = oc.orc_type == ORCGPU_T_BYTE || oc.orc_type == ORCGPU_T_SHORT || oc.orc_type == ORCGPU_T_INT || oc.orc_type == ORCGPU_T_LONG || oc.orc_type == ORCGPU_T_DATE;
  return is_int && (oc.width == 1 || oc.width == 2 || oc.width == 4 || oc.width == 8);
}

ComputedTable computed_table_layout(size_t n_file, size_t n, size_t n_ops, size_t n_segs) {
  ComputedTable t;
  Bump tb;
  t.o_cols = tb.take(n_file * sizeof(FilterCol) + 16, 16);
  t.o_jobs = tb.take(n * sizeof(ComputeJob) + 16, 16);
  t.o_ops = tb.take(n_ops * sizeof(AggExprOp) + 16, 16);
  t.o_segs = tb.take(n_segs * sizeof(SelBatch) + 16, 16);
  t.bytes = tb.off;
  return t;
}

// every operand of the plan against what the result's columns were decoded to
int computed_check_operands(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_host::ComputedPlan& plan, size_t n_file) {
  for (const AggExprOp& op : plan.ops) {
    if (op.op > AX_PUSH_F64) continue;  // (a gate or a push: `col` is a column of the result)
    if (op.col >= n_file || (op.op != AX_GATE && !computed_operand_fits(r->cols[op.col], op.op))) {
      set_err(ctx, "computed columns: column %u of the stripe is not decoded to the type the expression was planned for", op.col < n_file ? r->cols[op.col].column_id : op.col);
      return ORCGPU_MISMATCHED_SCHEMA;
    }
  }
  return ORCGPU_OK;
}

// values and validity of the computed columns r->cols[n_file ..] behind `off` of the arena of `lane`; returns the end
uint64_t computed_place_columns(orcgpu_result* r, size_t n_file, int lane, Bump& RB) {
  for (size_t k = n_file; k < r->cols.size(); k++) {
    ColumnOut& co = r->cols[k];
    co.lane = lane;
    co.values_bytes = r->n_rows * co.width;
    co.values_off = RB.take(co.values_bytes + 16);
    co.validity_off = RB.take((uint64_t)r->n_batches * r->words_per_batch * 8 + 16);
    co.null_counts.assign(r->n_batches, 0);
    co.status = 0;
  }
  return RB.off;
}

// The tables filled and uploaded to T, the kernel enqueued on `st`.  d_counts: n x n_batches null counts, then the overflow count,
// zero.  sel: the row selection's batches the count is restricted to (null: every row counts)
int computed_enqueue(orcgpu_ctx* ctx, hipStream_t st, orcgpu_result* r, const orcgpu_host::ComputedPlan& plan, size_t n_file, uint8_t* T, const ComputedTable& tab,
                     unsigned long long* d_counts, const std::vector<SelBatch>* sel) {
  const size_t n = plan.cols.size();
  std::vector<uint8_t> host(tab.bytes, 0);
  FilterCol* fcols = reinterpret_cast<FilterCol*>(host.data() + tab.o_cols);
  for (size_t c = 0; c < n_file; c++) {  // (what the programs do not read stays zero: no pointer, never loaded from)
    const ColumnOut& oc = r->cols[c];
    bool read = false;
    for (const AggExprOp& op : plan.ops) read = read || (op.op <= AX_PUSH_F64 && op.col == c);
    if (!read) continue;
    const uint8_t* A = r->arena[oc.lane].p;
    fcols[c].validity = oc.has_present ? reinterpret_cast<const unsigned long long*>(A + oc.validity_off) : nullptr;
    fcols[c].values = A + oc.values_off;
    fcols[c].width = oc.width;
    fcols[c].kind = oc.orc_type == ORCGPU_T_DECIMAL ? FKIND_DEC128 : (oc.orc_type == ORCGPU_T_FLOAT || oc.orc_type == ORCGPU_T_DOUBLE) ? FKIND_FLOAT : FKIND_INT;
  }
  ComputeJob* jobs = reinterpret_cast<ComputeJob*>(host.data() + tab.o_jobs);
  for (size_t k = 0; k < n; k++) {
    const orcgpu_host::ComputedColumn& c = plan.cols[k];
    const ColumnOut& co = r->cols[n_file + k];
    uint8_t* const A = r->arena[co.lane].p;
    jobs[k].prog = reinterpret_cast<const AggExprOp*>(T + tab.o_ops) + c.first_op;
    jobs[k].n_ops = c.n_ops;
    jobs[k].kind = c.cls == orcgpu_host::XCLASS_FLOAT ? CK_F64 : c.cls == orcgpu_host::XCLASS_DEC ? CK_DEC128 : CK_INT64;
    jobs[k].out_values = A + co.values_off;
    jobs[k].out_validity = reinterpret_cast<unsigned long long*>(A + co.validity_off);
    jobs[k].null_counts = d_counts + k * r->n_batches;
    jobs[k].overflow_rows = d_counts + n * r->n_batches;
  }
  memcpy(host.data() + tab.o_ops, plan.ops.data(), plan.ops.size() * sizeof(AggExprOp));
  const size_t n_segs = sel ? sel->size() : 0;
  if (n_segs) memcpy(host.data() + tab.o_segs, sel->data(), n_segs * sizeof(SelBatch));
  HIP_TRY(ctx, ctx->upload(T, host.data(), host.size(), st));
  const uint64_t n_words = (uint64_t)r->n_batches * r->words_per_batch;
  hipLaunchKernelGGL(agg_ops_hold_conversion(plan.ops.data(), plan.ops.size()) ? compute_columns_conv_kernel : agg_ops_hold_conditional(plan.ops.data(), plan.ops.size()) ? compute_columns_cond_kernel : agg_ops_hold_division(plan.ops.data(), plan.ops.size()) ? compute_columns_div_kernel : compute_columns_kernel, dim3((uint32_t)((n_words + 3) / 4), (uint32_t)n), dim3(256), 0, st, reinterpret_cast<const ComputeJob*>(T + tab.o_jobs),
                     reinterpret_cast<const FilterCol*>(T + tab.o_cols), (uint32_t)n_file, r->n_rows, r->n_batches, r->batch, r->words_per_batch,
                     reinterpret_cast<const SelBatch*>(T + tab.o_segs), (uint32_t)n_segs, sel ? 0u : 1u);
  HIP_TRY(ctx, hipGetLastError());
  return ORCGPU_OK;
}

int computed_plan_stripe(LaneRun& R, uint32_t si) {
  orcgpu_staged* s = R.stripes[si];
  if (!s->computed) return ORCGPU_OK;
  orcgpu_result* r = R.results[si];
  Plan& P = R.P;
  const orcgpu_host::ComputedPlan& plan = *s->computed;
  // (the columns in front of the computed ones: the file's, then the lookup columns -- which no program reads)
  const size_t n_file = s->cols.size() + (s->lookup ? s->lookup->cols.size() : 0), n = plan.cols.size();
  if (R.mask || r->cols.size() != n_file + n) {
    set_err(R.ctx, "computed columns: the decode call is not laid out for them");
    return ORCGPU_UNEXPECTED;
  }
  if (const int rc = computed_check_operands(R.ctx, r, plan, n_file)) return rc;
  LaneRun::ComputedPlace place;
  place.stripe = si;
  place.first_col = (uint32_t)n_file;
  place.nullcount_off = (uint32_t)P.n_nullcount_slots;
  P.n_nullcount_slots += (uint64_t)n * r->n_batches + 1;  // (the last: the stripe's overflow count)
  computed_place_columns(r, n_file, P.lane_id, P.result_bump[si]);
  place.tab = computed_table_layout(n_file, n, plan.ops.size(), s->has_sel ? s->sel.size() : 0);
  place.table_off = P.scratch.take(place.tab.bytes);
  R.computed.push_back(place);
  return ORCGPU_OK;
}

int computed_launch(LaneRun& R) {
  for (const LaneRun::ComputedPlace& place : R.computed) {
    orcgpu_staged* s = R.stripes[place.stripe];
    orcgpu_result* r = R.results[place.stripe];
    if (!r->n_rows || !r->n_batches) continue;
    // (the reader's row selection on these rows is known before the call: the overflow count is of the selected rows)
    if (const int rc = computed_enqueue(R.ctx, R.st, r, *s->computed, place.first_col, R.S + place.table_off, place.tab, R.d_nullc + place.nullcount_off,
                                        s->has_sel ? &s->sel : nullptr))
      return rc;
  }
  return ORCGPU_OK;
}

void computed_resolve(LaneRun& R) {
  const unsigned long long* h_nullc = R.h_nullc();
  for (const LaneRun::ComputedPlace& place : R.computed) {
    orcgpu_result* r = R.results[place.stripe];
    const size_t n = r->cols.size() - place.first_col;
    for (size_t k = 0; k < n; k++) {
      ColumnOut& co = r->cols[place.first_col + k];
      for (uint32_t b = 0; b < r->n_batches; b++) co.null_counts[b] = h_nullc[place.nullcount_off + k * r->n_batches + b];
    }
    r->computed_overflow = h_nullc[place.nullcount_off + n * r->n_batches];
  }
}

// The same on a decoded result, for a caller that decoded by hand: the columns appended behind the result's own, in lane 0's
// arena (grown, its contents kept, when the decode left no room behind them), evaluated on the decode stream; ONE wait of its own
// brings the counts back.  Before any row selection or row filter on the result; a result whose decode failed is left alone.
int result_compute_columns(orcgpu_ctx* ctx, orcgpu_result* r, const char* const* names, const orcgpu_agg_expr* exprs, uint32_t n, const char* const* column_names,
                           uint64_t* overflow_rows) {
  if (overflow_rows) *overflow_rows = 0;
  if (r->status) return r->status;
  if ((r->hold && orcgpu_hold::hold_exported(r->hold)) || r->selected || r->filtered) {
    set_err(ctx, "computed columns: the result has been selected on, filtered or exported: compute its columns first");
    return ORCGPU_INVALID_ARGUMENT;
  }
  const size_t n_file = r->cols.size();
  std::vector<orcgpu_host::AggExprCol> xcols(n_file);
  std::vector<uint8_t> nested(n_file, 0);
  for (size_t c = 0; c < n_file; c++) {
    const ColumnOut& co = r->cols[c];
    if (co.computed) {
      set_err(ctx, "computed columns: the result already holds computed columns");
      return ORCGPU_INVALID_ARGUMENT;
    }
    nested[c] = co.is_struct || co.is_union || co.is_list || co.elem || co.parent >= 0;
    orcgpu_host::AggExprCol& x = xcols[c];
    x.orc_type = co.orc_type;
    x.scale = co.scale;
    x.dict_out = co.dict_out;
    const int cls = orcgpu_host::agg_class(co.orc_type);
    x.fkind = co.is_string || co.is_bool ? FKIND_OTHER : cls == orcgpu_host::ACLASS_FLOAT ? FKIND_FLOAT : cls == orcgpu_host::ACLASS_DEC ? FKIND_DEC128
            : (cls == orcgpu_host::ACLASS_INT || cls == orcgpu_host::ACLASS_DATE) ? FKIND_INT : FKIND_OTHER;
  }
  orcgpu_host::ComputedPlan plan;
  if (const int rc = orcgpu_host::computed_compile(names, exprs, n, column_names, (uint32_t)n_file, column_names, xcols.data(), nested.data(), (uint32_t)n_file, plan)) {
    set_err(ctx, "%s", plan.err);
    return rc;
  }
  if (const int rc = computed_check_operands(ctx, r, plan, n_file)) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  orcgpu_staged shape;  // (what computed_append_columns reads of a staged stripe: the plan)
  shape.computed = std::make_shared<const orcgpu_host::ComputedPlan>(plan);
  computed_append_columns(&shape, r);
  Bump RB;
  RB.off = r->arena_used[0];
  const uint64_t need = computed_place_columns(r, n_file, 0, RB);
  DevBuf old;
  if (need + kAlign > r->arena[0].cap) {  // grow lane 0's arena: a new one, the decode's bytes copied over
    DevBuf grown;
    if (!grown.ensure(need + kAlign)) {
      r->cols.resize(n_file);
      set_err(ctx, "hipMalloc(%llu) for the computed columns failed", (unsigned long long)need);
      return ORCGPU_HIP_ERROR;
    }
    if (r->arena_used[0]) HIP_TRY(ctx, hipMemcpyAsync(grown.p, r->arena[0].p, r->arena_used[0], hipMemcpyDeviceToDevice, st));
    old = r->arena[0];
    r->arena[0] = grown;
  }
  r->arena_used[0] = need;
  const size_t n_counts = (size_t)n * r->n_batches + 1;
  std::vector<unsigned long long> back(n_counts, 0);
  int rc = ORCGPU_OK;
  if (r->n_rows && r->n_batches) {
    const ComputedTable tab = computed_table_layout(n_file, n, plan.ops.size(), 0);
    const uint64_t o_counts = align_up(tab.bytes, 16);
    if (!r->filt_tmp.ensure(o_counts + n_counts * 8 + kAlign)) {
      set_err(ctx, "hipMalloc for the computed columns' tables failed");
      rc = ORCGPU_HIP_ERROR;
    }
    uint8_t* T = r->filt_tmp.p;
    unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(T + o_counts);
    if (!rc && hipMemsetAsync(d_counts, 0, n_counts * 8, st) != hipSuccess) rc = ORCGPU_HIP_ERROR;
    if (!rc) rc = computed_enqueue(ctx, st, r, plan, n_file, T, tab, d_counts, nullptr);
    if (!rc && hipMemcpyAsync(back.data(), d_counts, n_counts * 8, hipMemcpyDeviceToHost, st) != hipSuccess) rc = ORCGPU_HIP_ERROR;
  }
  // ---- the call's one wait: the null counts and the overflow count ----
  if (hipStreamSynchronize(st) != hipSuccess && !rc) rc = ORCGPU_HIP_ERROR;
  old.release();
  if (rc) {
    if (rc == ORCGPU_HIP_ERROR) set_err(ctx, "computed columns: a HIP call failed");
    r->cols.resize(n_file);
    return rc;
  }
  for (size_t k = 0; k < n; k++) {
    ColumnOut& co = r->cols[n_file + k];
    for (uint32_t b = 0; b < r->n_batches; b++) co.null_counts[b] = back[k * r->n_batches + b];
    r->arrow_bytes += result_column_bytes(r, co);
  }
  r->computed_overflow = back[n_counts - 1];
  if (overflow_rows) *overflow_rows = r->computed_overflow;
  r->mirror_valid = false;
  r->dev_ready_recorded = false;
  return ORCGPU_OK;
}

}  // namespace

extern "C" int orcgpu_result_compute_columns(orcgpu_ctx* ctx, orcgpu_result* result, const char* const* names, const orcgpu_agg_expr* exprs, uint32_t n,
                                             const char* const* column_names, uint64_t* overflow_rows) {
  if (!ctx || !result || !column_names) return ORCGPU_INVALID_ARGUMENT;
  return result_compute_columns(ctx, result, names, exprs, n, column_names, overflow_rows);
}
