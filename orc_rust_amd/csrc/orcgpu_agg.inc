// orcgpu_agg.inc -- aggregates over the kept rows at the seam: orcgpu_result_aggregate and what the file reader calls per stripe.
// The plan compiler and the records' arithmetic are orcgpu_agg_plan.inc (host only), the kernels device/agg_kernels.hip; the
// filter's call (orcgpu_filter.inc) lends its FilterCall, its workspace and the front of its pipeline up to the evaluation.
//
// One aggregated result costs ONE host wait: upload -> LIKE / IN plane kernels -> filter_eval_kernel (its keep mask and nothing
// after it) -> agg_partial_kernel -> agg_final_kernel -> the wait, which fetches one record per aggregate and the kept row count.
// Without a filter nothing is evaluated: the partial kernel takes every input row as kept.  The result is read, never changed.
//
// Instructions that sum an arithmetic expression (AK_EXPR_*) bring their programs in an op table uploaded beside the instructions;
// agg_expr_partial_kernel / agg_group_expr_partial_kernel reduce them behind the plain partial kernel, into the same records, and
// are launched only when the list holds such an instruction.
//
// With a GROUP BY (orcgpu_result_aggregate_groups; orcgpu_group_plan.inc, device/agg_group_kernels.hip) the same front, then: zero
// the table -> group_assign_kernel -> group_number_kernel -> agg_group_partial_kernel -> agg_group_final_kernel -> the one wait,
// which fetches the group count and the flags, the key records and the value records in one copy.
#include "orcgpu_agg_plan.inc"
#include "orcgpu_group_plan.inc"
namespace {

// Where the aggregation's own tables lie: behind the filter's workspace, in the same allocation
struct AggWorkspace {
  uint32_t n_insn = 0, blocks = 0;  // instructions (the aggregates, then the kept row count); agg_partial_kernel's blocks along x
  uint64_t o_insn = 0, o_ops = 0, o_part = 0, o_out = 0, bytes = 0;
  AggWorkspace(uint64_t filter_bytes, uint32_t n_specs, uint64_t n_in, size_t n_ops) {
    FilterBump t;
    t.off = filter_bytes;
    n_insn = n_specs + 1;
    blocks = agg_blocks(n_in);
    o_insn = t.take((uint64_t)n_insn * sizeof(AggInsn) + 16);
    o_ops = t.take((uint64_t)n_ops * sizeof(AggExprOp) + 16);
    o_part = t.take((uint64_t)n_insn * blocks * sizeof(AggPartial) + 16);
    o_out = t.take((uint64_t)n_insn * sizeof(AggPartial) + 16);
    bytes = t.off;
  }
};

// Where the grouped aggregation's tables lie: behind the filter's workspace, in the same allocation.  [o_table, o_back) is zeroed
// on the stream before every call; [o_back, o_back + back_bytes) is what the one wait fetches: control, key records, value records
struct GroupWorkspace {
  uint32_t n_insn = 0, n_keys = 0, blocks = 0;
  uint64_t o_insn = 0, o_ops = 0, o_table = 0, zero_bytes = 0, o_plane = 0, o_slot_group = 0, o_part = 0, o_back = 0, back_keys = 0, back_vals = 0, back_bytes = 0, first = 0, bytes = 0;
  GroupWorkspace(uint64_t filter_bytes, uint32_t n_specs, uint32_t n_keys_, uint64_t n_in, size_t n_ops) {
    FilterBump t;
    t.off = filter_bytes;
    n_insn = n_specs + 1;
    n_keys = n_keys_;
    blocks = agg_group_blocks(n_in);
    first = o_insn = t.take((uint64_t)n_insn * sizeof(AggInsn) + 16);
    o_ops = t.take((uint64_t)n_ops * sizeof(AggExprOp) + 16);
    o_table = t.take((uint64_t)kGroupSlots * sizeof(GroupSlot));
    zero_bytes = (uint64_t)kGroupSlots * sizeof(GroupSlot);
    o_plane = t.take((n_in + 63) / 64 * 64 * 4 + 16);
    o_slot_group = t.take((uint64_t)kGroupSlots * 4 + 16);
    o_part = t.take((uint64_t)n_insn * blocks * kGroupMax * sizeof(AggPartial) + 16);
    back_keys = sizeof(GroupControl);
    back_vals = back_keys + (uint64_t)kGroupMax * n_keys * sizeof(GroupKeyRecord);
    back_bytes = back_vals + (uint64_t)n_insn * kGroupMax * sizeof(AggPartial);
    o_back = t.take(back_bytes + 16);
    bytes = t.off;
  }
};

// Do the instructions read what is there?  A column index below nc; a program inside the op table whose every op names a column
// below nc.  (The plan was compiled against these columns: anything else is a caller's mix-up.)
bool agg_plan_in_bounds(const std::vector<AggInsn>& insns, const std::vector<AggExprOp>& ops, uint32_t nc) {
  for (const AggInsn& in : insns) {
    if (in.kind == AK_COUNT_ROWS) continue;
    if (!agg_is_expr(in.kind)) {
      if (in.kind >= AK_N || in.col >= nc || in.col2 >= nc) return false;
      continue;
    }
    if (in.col > ops.size() || in.col2 > ops.size() - in.col || !in.col2) return false;
    for (uint32_t k = in.col; k < in.col + in.col2; k++)
      if (ops[k].op >= AX_N || (ops[k].op <= AX_PUSH_F64 && ops[k].col >= nc)) return false;
  }
  return true;
}

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
int agg_run(FilterCall& f, const FilterWorkspace& ws, const AggWorkspace& aw, const std::vector<AggInsn>& insns, const std::vector<AggExprOp>& ops, bool has_filter,
            AggPartial* records) {
  orcgpu_ctx* ctx = f.ctx;
  hipStream_t st = ctx->stream;
  const AggInsn* d_insn = f.at<const AggInsn>(aw.o_insn);
  AggPartial *d_part = f.at<AggPartial>(aw.o_part), *d_out = f.at<AggPartial>(aw.o_out);
  HIP_TRY(ctx, ctx->upload(f.X + aw.o_insn, insns.data(), insns.size() * sizeof(AggInsn), st));
  hipLaunchKernelGGL(agg_partial_kernel, dim3(aw.blocks, aw.n_insn), dim3(256), 0, st, d_insn, f.at<const FilterCol>(ws.o_cols), f.at<const SelBatch>(ws.o_segs),
                     f.at<const unsigned long long>(ws.o_first), (uint32_t)f.segs.size(), f.n_in, f.B, f.W,
                     has_filter ? f.at<const unsigned long long>(ws.o_keep) : nullptr, d_part);
  HIP_TRY(ctx, hipGetLastError());
  if (!ops.empty()) {  // the expression instructions' rows of the same records
    HIP_TRY(ctx, ctx->upload(f.X + aw.o_ops, ops.data(), ops.size() * sizeof(AggExprOp), st));
    hipLaunchKernelGGL(agg_expr_partial_kernel, dim3(aw.blocks, aw.n_insn), dim3(256), 0, st, d_insn, f.at<const AggExprOp>(aw.o_ops), f.at<const FilterCol>(ws.o_cols),
                       f.at<const SelBatch>(ws.o_segs), f.at<const unsigned long long>(ws.o_first), (uint32_t)f.segs.size(), f.n_in, f.B, f.W,
                       has_filter ? f.at<const unsigned long long>(ws.o_keep) : nullptr, d_part);
    HIP_TRY(ctx, hipGetLastError());
  }
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
  const AggWorkspace aw(ws.bytes, (uint32_t)aplan.insns.size(), f.n_in, aplan.ops.size());
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
  if (!agg_plan_in_bounds(insns, aplan.ops, f.nc)) return ORCGPU_UNEXPECTED;
  AggInsn kept{};
  kept.kind = AK_COUNT_ROWS;
  insns.push_back(kept);
  if (!f.n_in) return ORCGPU_OK;  // (no input row: every record is the empty one)
  if (const int rc = filter_upload(f, ws, host)) return rc;
  if (fplan)
    if (const int rc = filter_run_eval(f, ws)) return rc;
  if (const int rc = agg_run(f, ws, aw, insns, aplan.ops, fplan != nullptr, records.data())) return rc;
  if (records.back().w[0] > f.n_in) {
    set_err(ctx, "aggregate: %llu rows kept of %llu", (unsigned long long)records.back().w[0], (unsigned long long)f.n_in);
    return ORCGPU_UNEXPECTED;
  }
  return ORCGPU_OK;
}

// The plan of an aggregate list against a decoded result's columns
int result_compile_aggs(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_agg_spec* specs, const orcgpu_agg_expr* exprs, uint32_t n_specs,
                        const char* const* column_names, orcgpu_host::AggPlan& plan) {
  std::vector<FilterColDesc> descs;
  for (const ColumnOut& co : r->cols) descs.push_back(filter_desc_of(co));
  std::vector<orcgpu_host::AggCol> cols;
  agg_describe(r, descs, cols);
  const int rc = orcgpu_host::agg_compile(specs, exprs, n_specs, column_names, cols.data(), (uint32_t)cols.size(), plan);
  if (rc) set_err(ctx, "%s", plan.err);
  return rc;
}

// The grouped reduction behind the evaluation and its one wait: `set` gets the result's groups in first-appearance order, with
// the instructions' records and behind them the group's kept row count
int group_run(FilterCall& f, const FilterWorkspace& ws, const GroupWorkspace& gw, const orcgpu_host::GroupPlan& gplan, const std::vector<AggInsn>& insns,
              const std::vector<AggExprOp>& ops, bool has_filter, const char* const* column_names, orcgpu_host::GroupSet& set) {
  orcgpu_ctx* ctx = f.ctx;
  hipStream_t st = ctx->stream;
  GroupKeys keys{};
  keys.n = (uint32_t)gplan.keys.size();
  keys.hash_mask = orcgpu_host::group_hash_mask(getenv("ORCGPU_GROUP_HASH_BITS"));
  for (uint32_t k = 0; k < keys.n; k++) {
    keys.col[k] = gplan.keys[k].col;
    keys.fkind[k] = gplan.keys[k].fkind;
  }
  const AggInsn* d_insn = f.at<const AggInsn>(gw.o_insn);
  const FilterCol* d_cols = f.at<const FilterCol>(ws.o_cols);
  const SelBatch* d_segs = f.at<const SelBatch>(ws.o_segs);
  const unsigned long long* d_first = f.at<const unsigned long long>(ws.o_first);
  const unsigned long long* d_keep = has_filter ? f.at<const unsigned long long>(ws.o_keep) : nullptr;
  GroupSlot* d_table = f.at<GroupSlot>(gw.o_table);
  GroupControl* d_ctl = f.at<GroupControl>(gw.o_back);
  uint32_t *d_plane = f.at<uint32_t>(gw.o_plane), *d_slot_group = f.at<uint32_t>(gw.o_slot_group);
  GroupKeyRecord* d_keys = f.at<GroupKeyRecord>(gw.o_back + gw.back_keys);
  AggPartial *d_part = f.at<AggPartial>(gw.o_part), *d_out = f.at<AggPartial>(gw.o_back + gw.back_vals);
  const uint32_t n_segs = (uint32_t)f.segs.size();
  {
    // (the debugging aid of the decode: nothing here may depend on what the workspace held before)
    static const char* poison = getenv("ORCGPU_POISON");
    if (poison && *poison) HIP_TRY(ctx, hipMemsetAsync(f.X + gw.first, (int)strtol(poison, nullptr, 0) & 0xFF, gw.bytes - gw.first, st));
  }
  HIP_TRY(ctx, ctx->upload(f.X + gw.o_insn, insns.data(), insns.size() * sizeof(AggInsn), st));
  HIP_TRY(ctx, hipMemsetAsync(d_table, 0, gw.zero_bytes, st));
  HIP_TRY(ctx, hipMemsetAsync(d_ctl, 0, gw.back_bytes, st));
  hipLaunchKernelGGL(group_assign_kernel, dim3(gw.blocks), dim3(256), 0, st, keys, d_cols, d_segs, d_first, n_segs, f.n_in, f.B, f.W, d_keep, d_table, d_ctl, d_plane);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(group_number_kernel, dim3(1), dim3(kGroupSlots), 0, st, keys, d_cols, d_segs, d_first, n_segs, f.n_in, f.B, f.W, d_table, d_ctl, d_slot_group, d_keys);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(agg_group_partial_kernel, dim3(gw.blocks, gw.n_insn), dim3(256), 0, st, d_insn, d_cols, d_segs, d_first, n_segs, f.n_in, f.B, f.W, d_keep, d_plane,
                     d_slot_group, d_ctl, d_part);
  HIP_TRY(ctx, hipGetLastError());
  if (!ops.empty()) {  // the expression instructions' rows of the same records
    HIP_TRY(ctx, ctx->upload(f.X + gw.o_ops, ops.data(), ops.size() * sizeof(AggExprOp), st));
    hipLaunchKernelGGL(agg_group_expr_partial_kernel, dim3(gw.blocks, gw.n_insn), dim3(256), 0, st, d_insn, f.at<const AggExprOp>(gw.o_ops), d_cols, d_segs, d_first, n_segs,
                       f.n_in, f.B, f.W, d_keep, d_plane, d_slot_group, d_ctl, d_part);
    HIP_TRY(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(agg_group_final_kernel, dim3(kGroupMax, gw.n_insn), dim3(256), 0, st, d_insn, d_part, gw.blocks, d_ctl, d_out);
  HIP_TRY(ctx, hipGetLastError());
  // ---- the grouped aggregation's one wait: the group count and the flags, the key records, the value records ----
  std::vector<uint8_t> back(gw.back_bytes);
  HIP_TRY(ctx, hipMemcpyAsync(back.data(), d_ctl, gw.back_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  GroupControl ctl;
  memcpy(&ctl, back.data(), sizeof(ctl));
  char err[256];
  if (const int rc = orcgpu_host::group_check_flags(gplan, ctl.flags, ctl.n_groups, column_names, err, sizeof(err))) {
    set_err(ctx, "%s", err);
    return rc;
  }
  const uint32_t n = ctl.n_groups, nk = keys.n, ni = gw.n_insn;
  set.n_keys = nk;
  set.n_insn = ni;
  set.keys.resize((size_t)n * nk);
  set.vals.resize((size_t)n * ni);
  if (n) memcpy(set.keys.data(), back.data() + gw.back_keys, (size_t)n * nk * sizeof(GroupKeyRecord));
  const AggPartial* vals = reinterpret_cast<const AggPartial*>(back.data() + gw.back_vals);  // [instruction][kGroupMax]
  for (uint32_t g = 0; g < n; g++)
    for (uint32_t k = 0; k < ni; k++) set.vals[(size_t)g * ni + k] = vals[(size_t)k * kGroupMax + g];
  return ORCGPU_OK;
}

// result_aggregate_plan with a GROUP BY: `set` gets the groups of the kept rows, every group's records and behind them its kept
// row count; *rows_kept their sum
int result_aggregate_groups_plan(orcgpu_ctx* ctx, const orcgpu_result* r_, const orcgpu_host::FilterPlan* fplan, const orcgpu_host::AggPlan& aplan,
                                 const orcgpu_host::GroupPlan& gplan, orcgpu_host::GroupSet& set, uint64_t* rows_seen, uint64_t* rows_kept,
                                 const char* const* column_names, uint32_t n_names) {
  static const orcgpu_host::FilterPlan no_filter;
  orcgpu_result* r = const_cast<orcgpu_result*>(r_);  // (what is written is the filter's scratch allocation, never a batch)
  set = orcgpu_host::GroupSet{};
  set.n_keys = (uint32_t)gplan.keys.size();
  set.n_insn = (uint32_t)aplan.insns.size() + 1;
  if (rows_seen) *rows_seen = 0;
  if (rows_kept) *rows_kept = 0;
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
  const GroupWorkspace gw(ws.bytes, (uint32_t)aplan.insns.size(), (uint32_t)gplan.keys.size(), f.n_in, aplan.ops.size());
  if (!r->filt_tmp.ensure(gw.bytes + kAlign)) {
    set_err(ctx, "hipMalloc(%llu) for the grouped aggregation failed", (unsigned long long)gw.bytes);
    return ORCGPU_HIP_ERROR;
  }
  f.X = r->filt_tmp.p;
  std::vector<uint8_t> host(ws.up_bytes, 0);
  filter_fill_cols(f, ws, src_batches, host.data());
  if (fplan)
    if (const int rc = filter_check(f, column_names, n_names)) return rc;
  std::vector<AggInsn> insns = aplan.insns;
  if (!agg_plan_in_bounds(insns, aplan.ops, f.nc)) return ORCGPU_UNEXPECTED;
  for (const orcgpu_host::GroupKey& k : gplan.keys)
    if (k.col >= f.nc || k.col >= n_names || f.fcols[k.col].kind != k.fkind) return ORCGPU_UNEXPECTED;
  AggInsn kept{};
  kept.kind = AK_COUNT_ROWS;
  insns.push_back(kept);
  if (!f.n_in) return ORCGPU_OK;  // (no input row: no group)
  if (const int rc = filter_upload(f, ws, host)) return rc;
  if (fplan)
    if (const int rc = filter_run_eval(f, ws)) return rc;
  if (const int rc = group_run(f, ws, gw, gplan, insns, aplan.ops, fplan != nullptr, column_names, set)) return rc;
  uint64_t total = 0;
  for (uint32_t g = 0; g < set.n_groups(); g++) total += set.vals[(size_t)g * set.n_insn + set.n_insn - 1].w[0];
  if (total > f.n_in) {
    set_err(ctx, "group by: %llu rows kept of %llu", (unsigned long long)total, (unsigned long long)f.n_in);
    return ORCGPU_UNEXPECTED;
  }
  if (rows_kept) *rows_kept = total;
  return ORCGPU_OK;
}

// The plan of a key list against a decoded result's columns
int result_compile_group(orcgpu_ctx* ctx, const orcgpu_result* r, const char* const* key_columns, uint32_t n_keys, const char* const* column_names,
                         orcgpu_host::GroupPlan& plan) {
  std::vector<FilterColDesc> descs;
  for (const ColumnOut& co : r->cols) descs.push_back(filter_desc_of(co));
  std::vector<orcgpu_host::AggCol> cols;
  agg_describe(r, descs, cols);
  const int rc = orcgpu_host::group_compile(key_columns, n_keys, column_names, cols.data(), (uint32_t)cols.size(), plan);
  if (rc) set_err(ctx, "%s", plan.err);
  return rc;
}

}  // namespace

extern "C" int orcgpu_result_aggregate(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                       const char* const* column_names, uint32_t n_columns, const orcgpu_agg_spec* specs, uint32_t n_specs,
                                       orcgpu_agg_value* out) {
  return orcgpu_result_aggregate_exprs(ctx, r, nodes, n_nodes, column_names, n_columns, specs, nullptr, n_specs, out);
}
extern "C" int orcgpu_result_aggregate_exprs(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                             const char* const* column_names, uint32_t n_columns, const orcgpu_agg_spec* specs,
                                             const orcgpu_agg_expr* exprs, uint32_t n_specs, orcgpu_agg_value* out) {
  if (!ctx || !r || (n_nodes && !nodes) || (n_columns && !column_names) || !out) return ORCGPU_INVALID_ARGUMENT;
  if (r->status) return r->status;
  if (n_columns != r->cols.size()) {
    set_err(ctx, "aggregate: %u column names for a result of %zu columns", n_columns, r->cols.size());
    return ORCGPU_INVALID_ARGUMENT;
  }
  orcgpu_host::AggPlan aplan;
  if (const int rc = result_compile_aggs(ctx, r, specs, exprs, n_specs, column_names, aplan)) return rc;
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

extern "C" int orcgpu_result_aggregate_groups(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                              const char* const* column_names, uint32_t n_columns, const char* const* key_columns, uint32_t n_keys,
                                              const orcgpu_agg_spec* specs, uint32_t n_specs, orcgpu_groups** out) {
  return orcgpu_result_aggregate_groups_exprs(ctx, r, nodes, n_nodes, column_names, n_columns, key_columns, n_keys, specs, nullptr, n_specs, out);
}
extern "C" int orcgpu_result_aggregate_groups_exprs(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                                    const char* const* column_names, uint32_t n_columns, const char* const* key_columns, uint32_t n_keys,
                                                    const orcgpu_agg_spec* specs, const orcgpu_agg_expr* exprs, uint32_t n_specs, orcgpu_groups** out) {
  if (out) *out = nullptr;
  if (!ctx || !r || (n_nodes && !nodes) || (n_columns && !column_names) || !out) return ORCGPU_INVALID_ARGUMENT;
  if (r->status) return r->status;
  if (n_columns != r->cols.size()) {
    set_err(ctx, "group by: %u column names for a result of %zu columns", n_columns, r->cols.size());
    return ORCGPU_INVALID_ARGUMENT;
  }
  orcgpu_host::GroupPlan gplan;
  if (const int rc = result_compile_group(ctx, r, key_columns, n_keys, column_names, gplan)) return rc;
  orcgpu_host::AggPlan aplan;
  if (const int rc = result_compile_aggs(ctx, r, specs, exprs, n_specs, column_names, aplan)) return rc;
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
  orcgpu_host::GroupSet set;
  if (const int rc = result_aggregate_groups_plan(ctx, r, n_nodes ? &fplan : nullptr, aplan, gplan, set, nullptr, nullptr, column_names, n_columns)) return rc;
  std::vector<AggInsn> insns = aplan.insns;
  insns.push_back(AggInsn{});
  orcgpu_groups* g = new orcgpu_groups;
  orcgpu_host::group_finish(gplan, insns, n_specs, set, *g);
  *out = g;
  return ORCGPU_OK;
}
extern "C" uint32_t orcgpu_groups_count(const orcgpu_groups* g) { return g ? g->n_groups : 0; }
extern "C" int orcgpu_groups_key(const orcgpu_groups* g, uint32_t group, uint32_t key, orcgpu_group_key* out) {
  if (!g || !out || group >= g->n_groups || key >= g->n_keys) return ORCGPU_INVALID_ARGUMENT;
  *out = g->keys[(size_t)group * g->n_keys + key];
  return ORCGPU_OK;
}
extern "C" int orcgpu_groups_value(const orcgpu_groups* g, uint32_t group, uint32_t spec, orcgpu_agg_value* out) {
  if (!g || !out || group >= g->n_groups || spec >= g->n_specs) return ORCGPU_INVALID_ARGUMENT;
  *out = g->values[(size_t)group * g->n_specs + spec];
  return ORCGPU_OK;
}
extern "C" void orcgpu_groups_free(orcgpu_groups* g) { delete g; }
