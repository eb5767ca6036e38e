// orcgpu_agg.inc -- aggregates over the kept rows at the seam: orcgpu_result_aggregate and what the file reader calls per stripe.
// The plan compiler and the records' arithmetic are orcgpu_agg_plan.inc (host only), the kernels device/agg_kernels.hip; the
// filter's call (orcgpu_filter.inc) lends its FilterCall, its workspace and the front of its pipeline up to the evaluation.
//
// One aggregated result costs ONE host wait: upload -> LIKE / IN plane kernels -> filter_eval_kernel (its keep mask and nothing
// after it) -> agg_partial_kernel -> agg_final_kernel -> the wait, which fetches one record per aggregate and the kept row count.
// Without a filter nothing is evaluated: the partial kernel takes every input row as kept.  The result is read, never changed.
#include "orcgpu_agg_plan.inc"
namespace {

// Where the aggregation's own tables lie: behind the filter's workspace, in the same allocation
struct AggWorkspace {
  uint32_t n_insn = 0, blocks = 0;  // instructions (the aggregates, then the kept row count); agg_partial_kernel's blocks along x
  uint64_t o_insn = 0, o_part = 0, o_out = 0, bytes = 0;
  AggWorkspace(uint64_t filter_bytes, uint32_t n_specs, uint64_t n_in) {
    FilterBump t;
    t.off = filter_bytes;
    n_insn = n_specs + 1;
    blocks = agg_blocks(n_in);
    o_insn = t.take((uint64_t)n_insn * sizeof(AggInsn) + 16);
    o_part = t.take((uint64_t)n_insn * blocks * sizeof(AggPartial) + 16);
    o_out = t.take((uint64_t)n_insn * sizeof(AggPartial) + 16);
    bytes = t.off;
  }
};

void agg_describe(const orcgpu_result* r, const std::vector<FilterColDesc>& descs, std::vector<orcgpu_host::AggCol>& cols) {
  cols.resize(r->cols.size());
  for (size_t c = 0; c < r->cols.size(); c++) {
    const ColumnOut& co = r->cols[c];
    cols[c].d = descs[c];
    cols[c].scale = co.scale;
    cols[c].nested = co.is_struct || co.is_union || co.is_list || co.elem || co.parent >= 0;
  }
}

// Partial -> final -> the one wait: records[k] for instruction k
int agg_run(FilterCall& f, const FilterWorkspace& ws, const AggWorkspace& aw, const std::vector<AggInsn>& insns, bool has_filter, AggPartial* records) {
  orcgpu_ctx* ctx = f.ctx;
  hipStream_t st = ctx->stream;
  const AggInsn* d_insn = f.at<const AggInsn>(aw.o_insn);
  AggPartial *d_part = f.at<AggPartial>(aw.o_part), *d_out = f.at<AggPartial>(aw.o_out);
  HIP_TRY(ctx, ctx->upload(f.X + aw.o_insn, insns.data(), insns.size() * sizeof(AggInsn), st));
  hipLaunchKernelGGL(agg_partial_kernel, dim3(aw.blocks, aw.n_insn), dim3(256), 0, st, d_insn, f.at<const FilterCol>(ws.o_cols), f.at<const SelBatch>(ws.o_segs),
                     f.at<const unsigned long long>(ws.o_first), (uint32_t)f.segs.size(), f.n_in, f.B, f.W,
                     has_filter ? f.at<const unsigned long long>(ws.o_keep) : nullptr, d_part);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(agg_final_kernel, dim3(aw.n_insn), dim3(256), 0, st, d_insn, d_part, aw.blocks, d_out);
  HIP_TRY(ctx, hipGetLastError());
  // ---- the aggregation's one wait: a record per aggregate, and the kept row count ----
  HIP_TRY(ctx, hipMemcpyAsync(records, d_out, (size_t)aw.n_insn * sizeof(AggPartial), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return ORCGPU_OK;
}

// The rows of `r` that `fplan` keeps (null: all of them), reduced by `aplan`: records gets one per instruction of the plan and
// behind them the kept row count (in w[0]).  names: the result's columns, for the messages.
int result_aggregate_plan(orcgpu_ctx* ctx, const orcgpu_result* r_, const orcgpu_host::FilterPlan* fplan, const orcgpu_host::AggPlan& aplan,
                          std::vector<AggPartial>& records, uint64_t* rows_seen, const char* const* column_names, uint32_t n_names) {
  static const orcgpu_host::FilterPlan no_filter;
  orcgpu_result* r = const_cast<orcgpu_result*>(r_);  // (what is written is the filter's scratch allocation, never a batch)
  records.assign(aplan.insns.size() + 1, AggPartial{});
  if (rows_seen) *rows_seen = 0;
  if (r->status) return r->status;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  FilterCall f{ctx, r, fplan ? *fplan : no_filter};
  f.nc = (uint32_t)r->cols.size();
  f.B = r->batch;
  f.W = r->words_per_batch;
  filter_segments(f);
  filter_describe(f);
  if (rows_seen) *rows_seen = f.n_in;
  const uint32_t src_batches = r->selected ? r->full_batches : r->n_batches;
  const FilterWorkspace ws(f.plan, f.descs.data(), f.nc, (uint32_t)f.segs.size(), src_batches, f.n_in, f.B);
  const AggWorkspace aw(ws.bytes, (uint32_t)aplan.insns.size(), f.n_in);
  if (!r->filt_tmp.ensure(aw.bytes + kAlign)) {
    set_err(ctx, "hipMalloc(%llu) for the aggregation failed", (unsigned long long)aw.bytes);
    return ORCGPU_HIP_ERROR;
  }
  f.X = r->filt_tmp.p;
  std::vector<uint8_t> host(ws.up_bytes, 0);
  filter_fill_cols(f, ws, src_batches, host.data());
  if (fplan)
    if (const int rc = filter_check(f, column_names, n_names)) return rc;
  std::vector<AggInsn> insns = aplan.insns;
  for (const AggInsn& in : insns)  // (the plan was compiled against these columns: an index past them is a caller's mix-up)
    if (in.kind != AK_COUNT_ROWS && (in.col >= f.nc || in.col2 >= f.nc)) return ORCGPU_UNEXPECTED;
  AggInsn kept{};
  kept.kind = AK_COUNT_ROWS;
  insns.push_back(kept);
  if (!f.n_in) return ORCGPU_OK;  // (no input row: every record is the empty one)
  if (const int rc = filter_upload(f, ws, host)) return rc;
  if (fplan)
    if (const int rc = filter_run_eval(f, ws)) return rc;
  if (const int rc = agg_run(f, ws, aw, insns, fplan != nullptr, records.data())) return rc;
  if (records.back().w[0] > f.n_in) {
    set_err(ctx, "aggregate: %llu rows kept of %llu", (unsigned long long)records.back().w[0], (unsigned long long)f.n_in);
    return ORCGPU_UNEXPECTED;
  }
  return ORCGPU_OK;
}

// The plan of an aggregate list against a decoded result's columns
int result_compile_aggs(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_agg_spec* specs, uint32_t n_specs, const char* const* column_names,
                        orcgpu_host::AggPlan& plan) {
  std::vector<FilterColDesc> descs;
  for (const ColumnOut& co : r->cols) descs.push_back(filter_desc_of(co));
  std::vector<orcgpu_host::AggCol> cols;
  agg_describe(r, descs, cols);
  const int rc = orcgpu_host::agg_compile(specs, n_specs, column_names, cols.data(), (uint32_t)cols.size(), plan);
  if (rc) set_err(ctx, "%s", plan.err);
  return rc;
}

}  // namespace

extern "C" int orcgpu_result_aggregate(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                       const char* const* column_names, uint32_t n_columns, const orcgpu_agg_spec* specs, uint32_t n_specs,
                                       orcgpu_agg_value* out) {
  if (!ctx || !r || (n_nodes && !nodes) || (n_columns && !column_names) || !out) return ORCGPU_INVALID_ARGUMENT;
  if (r->status) return r->status;
  if (n_columns != r->cols.size()) {
    set_err(ctx, "aggregate: %u column names for a result of %zu columns", n_columns, r->cols.size());
    return ORCGPU_INVALID_ARGUMENT;
  }
  orcgpu_host::AggPlan aplan;
  if (const int rc = result_compile_aggs(ctx, r, specs, n_specs, column_names, aplan)) return rc;
  orcgpu_host::FilterPlan fplan;
  if (n_nodes) {
    std::vector<int32_t> kinds(n_columns), params(n_columns, 0);
    for (uint32_t c = 0; c < n_columns; c++) {
      const ColumnOut& co = r->cols[c];
      kinds[c] = co.orc_type;
      params[c] = co.orc_type == ORCGPU_T_DECIMAL ? (int32_t)co.scale : co.ts_unit;
    }
    const int rc = orcgpu_host::filter_compile(nodes, n_nodes, column_names, kinds.data(), n_columns, fplan, params.data());
    if (rc) {
      set_err(ctx, "%s", fplan.err);
      return rc;
    }
  }
  std::vector<AggPartial> records;
  if (const int rc = result_aggregate_plan(ctx, r, n_nodes ? &fplan : nullptr, aplan, records, nullptr, column_names, n_columns)) return rc;
  for (uint32_t k = 0; k < n_specs; k++) orcgpu_host::agg_finish(aplan.insns[k], records[k], &out[k]);
  return ORCGPU_OK;
}
