// orcgpu_agg.inc -- aggregates over the kept rows at the seam: orcgpu_result_aggregate, orcgpu_result_aggregate_groups and what the
// file reader calls per stripe.  The plan compilers and the records' arithmetic are orcgpu_agg_plan.inc and orcgpu_group_plan.inc
// (host only), the kernels device/agg_kernels.hip and device/agg_group_kernels.hip; the filter's call (orcgpu_filter.inc) lends its
// FilterCall, its workspace, its opening and the front of its pipeline up to the evaluation.
//
// Plain and grouped are ONE call, result_aggregate_call, with or without a GroupPlan; it costs ONE host wait.  Open -> reserve (the
// aggregation's tables lie behind the filter's: AggWorkspace) -> upload -> LIKE / IN plane kernels -> filter_eval_kernel (its keep
// mask and nothing after it; without a filter nothing is evaluated and every input row is kept) -> then
//   agg_run      agg_partial_kernel -> agg_final_kernel -> the wait, which fetches one record per instruction;
//   group_run    zero the table -> group_assign_kernel -> group_number_kernel -> agg_group_partial_kernel -> agg_group_final_kernel
//                -> the wait, which fetches the group count and the flags, the key records and the value records in one copy.
//   group_run_wide   (a GroupPlan whose max_groups is above kGroupMax: device/agg_group_wide_kernels.hip, its head comment has the
//                pipeline) zero the table -> assign -> count / scan / number -> the sort's passes -> segments -> the reduction ->
//                the FIRST wait, which fetches the control -> the flags check -> the SECOND, which fetches n_groups key and value
//                records.  Two waits, and nothing copied back that the limit sizes.
// The result is read, never changed.  The instructions are the plan's and, behind them, the kept row count (AK_COUNT_ROWS).
//
// Instructions that sum an arithmetic expression (AK_EXPR_*) bring their programs in an op table uploaded beside the instructions
// (agg_upload); agg_expr_partial_kernel / agg_group_expr_partial_kernel (a list that holds a division: their *_div_* twins) reduce them behind the plain partial kernel, into the same
// records, and are launched only when the list holds such an instruction (agg_launch_partials).  The six kernels that walk rows
// take them as one argument, KeptRows (filter_kept_rows).
//
// Aggregates with a condition (FILTER (WHERE ...): AggPlan::conds) bring their programs behind the row filter's in ONE predicate
// program (filter_plan_append), so that the filter's workspace, upload, kind check and plane kernels serve them as they are;
// agg_cond_eval_kernel then leaves one mask plane per distinct condition behind the keep mask and in front of the partial
// kernels, on the call's stream (agg_run_conds).  No further wait.
#include "orcgpu_agg_plan.inc"
#include "orcgpu_group_plan.inc"
namespace {

// Where the aggregation's own tables lie: behind the filter's workspace, in the same allocation.  [o_back, o_back + back_bytes) is
// what the one wait fetches: the value records [instruction] -- with a GROUP BY the control, the key records, then the value
// records [instruction][kGroupMax], and [o_table, o_table + zero_bytes) is zeroed on the stream before every call
struct AggWorkspace {
  uint32_t n_insn = 0, n_keys = 0, blocks = 0;  // instructions (the aggregates, then the kept row count); the partial kernel's blocks along x
  uint32_t n_conds = 0;  // distinct conditions: their spans in the predicate program, and a plane of ceil(n_in / 64) words each
  uint64_t o_spans = 0, o_cond = 0;
  uint64_t o_insn = 0, o_ops = 0, o_table = 0, zero_bytes = 0, o_plane = 0, o_slot_group = 0, o_part = 0, o_back = 0, back_keys = 0, back_vals = 0, back_bytes = 0, bytes = 0;
  orcgpu_host::GroupWideLayout wide;  // the wide path's tables instead (group_wide_layout), behind the instructions and the op table
  AggWorkspace(uint64_t filter_bytes, uint32_t n_specs, const orcgpu_host::GroupPlan* gplan, uint64_t n_in, size_t n_ops, size_t n_conds_ = 0) {
    FilterBump t;
    t.off = filter_bytes;
    n_insn = n_specs + 1;
    n_conds = (uint32_t)n_conds_;
    blocks = gplan ? agg_group_blocks(n_in) : agg_blocks(n_in);
    o_insn = t.take((uint64_t)n_insn * sizeof(AggInsn) + 16);
    o_ops = t.take((uint64_t)n_ops * sizeof(AggExprOp) + 16);
    if (n_conds) {
      o_spans = t.take((uint64_t)n_conds * sizeof(AggCondSpan) + 16);
      o_cond = t.take((uint64_t)n_conds * ((n_in + 63) / 64) * 8 + 16);
    }
    if (gplan && orcgpu_host::group_is_wide(gplan->max_groups)) {
      n_keys = (uint32_t)gplan->keys.size();
      blocks = agg_blocks(n_in);
      wide = orcgpu_host::group_wide_layout(t.off, gplan->max_groups, n_in, n_insn, n_keys);
      bytes = wide.bytes;
      return;
    }
    if (gplan) {
      n_keys = (uint32_t)gplan->keys.size();
      zero_bytes = (uint64_t)kGroupSlots * sizeof(GroupSlot);
      o_table = t.take(zero_bytes);
      o_plane = t.take((n_in + 63) / 64 * 64 * 4 + 16);
      o_slot_group = t.take((uint64_t)kGroupSlots * 4 + 16);
      back_keys = sizeof(GroupControl);
      back_vals = back_keys + (uint64_t)kGroupMax * n_keys * sizeof(GroupKeyRecord);
    }
    const uint64_t groups = gplan ? kGroupMax : 1;
    o_part = t.take((uint64_t)n_insn * blocks * groups * sizeof(AggPartial) + 16);
    back_bytes = back_vals + (uint64_t)n_insn * groups * sizeof(AggPartial);
    o_back = t.take(back_bytes + 16);
    bytes = t.off;
  }
};

// Do the keys read what is there (the instructions: agg_plan_in_bounds, orcgpu_agg_plan.inc)?  A column of the result, by name
// too, decoded to the kind the key was planned for
bool group_plan_in_bounds(const orcgpu_host::GroupPlan& gplan, const FilterCall& f) {
  for (const orcgpu_host::GroupKey& k : gplan.keys)
    if (k.col >= f.nc || k.col >= f.n_names || f.fcols[k.col].kind != k.fkind) return false;
  return true;
}

// A decoded result's columns as the plan compilers (agg_compile, group_compile) take them
std::vector<orcgpu_host::AggCol> result_agg_cols(const orcgpu_result* r) {
  std::vector<orcgpu_host::AggCol> cols(r->cols.size());
  for (size_t c = 0; c < r->cols.size(); c++) {
    const ColumnOut& co = r->cols[c];
    cols[c].d = filter_desc_of(co);
    cols[c].scale = co.scale;
    cols[c].nested = co.is_struct || co.is_union || co.is_list || co.elem || co.parent >= 0;
  }
  return cols;
}
// The plan of an aggregate list against a decoded result's columns
int result_compile_aggs(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_agg_spec* specs, const orcgpu_agg_expr* exprs, const orcgpu_agg_filter* filters,
                        uint32_t n_specs, const char* const* column_names, orcgpu_host::AggPlan& plan) {
  const std::vector<orcgpu_host::AggCol> cols = result_agg_cols(r);
  const orcgpu_host::KeySetRefs sets = ctx_key_set_refs(ctx);  // (what a condition's set leaf may name)
  const int rc = orcgpu_host::agg_compile(specs, exprs, filters, n_specs, column_names, cols.data(), (uint32_t)cols.size(), plan, &sets);
  if (rc) set_err(ctx, "%s", plan.err);
  return rc;
}
// The plan of a key list against a decoded result's columns
int result_compile_group(orcgpu_ctx* ctx, const orcgpu_result* r, const char* const* key_columns, uint32_t n_keys, const char* const* column_names,
                         orcgpu_host::GroupPlan& plan) {
  const std::vector<orcgpu_host::AggCol> cols = result_agg_cols(r);
  const int rc = orcgpu_host::group_compile(key_columns, n_keys, column_names, cols.data(), (uint32_t)cols.size(), plan);
  if (rc) set_err(ctx, "%s", plan.err);
  return rc;
}

// The instructions and the op table their programs lie in (none: nothing goes up for it), where the kernels read them
int agg_upload(const FilterCall& f, const AggWorkspace& aw, const std::vector<AggInsn>& insns, const std::vector<AggExprOp>& ops) {
  HIP_TRY(f.ctx, f.ctx->upload(f.X + aw.o_insn, insns.data(), insns.size() * sizeof(AggInsn), f.ctx->stream));
  HIP_TRY(f.ctx, f.ctx->upload(f.X + aw.o_ops, ops.data(), ops.size() * sizeof(AggExprOp), f.ctx->stream));
  return ORCGPU_OK;
}
// The partial kernels of a call, grid (blocks, instructions): the plain kinds', then -- only when the list holds an expression --
// the expression instructions' rows of the same records.  tail: what the pair takes behind the rows.
template <typename... Tail>
int agg_launch_partials(const FilterCall& f, const AggWorkspace& aw, bool has_exprs, void (*plain)(const AggInsn*, KeptRows, Tail...),
                        void (*expr)(const AggInsn*, const AggExprOp*, KeptRows, Tail...), const KeptRows& rows, Tail... tail) {
  const AggInsn* d_insn = f.at<const AggInsn>(aw.o_insn);
  hipLaunchKernelGGL(plain, dim3(aw.blocks, aw.n_insn), dim3(256), 0, f.ctx->stream, d_insn, rows, tail...);
  HIP_TRY(f.ctx, hipGetLastError());
  if (!has_exprs) return ORCGPU_OK;
  hipLaunchKernelGGL(expr, dim3(aw.blocks, aw.n_insn), dim3(256), 0, f.ctx->stream, d_insn, f.at<const AggExprOp>(aw.o_ops), rows, tail...);
  HIP_TRY(f.ctx, hipGetLastError());
  return ORCGPU_OK;
}

// Partial -> final -> the one wait: records[k] for instruction k
int agg_run(const FilterCall& f, const AggWorkspace& aw, const KeptRows& rows, const std::vector<AggInsn>& insns, const std::vector<AggExprOp>& ops,
            AggPartial* records) {
  orcgpu_ctx* ctx = f.ctx;
  hipStream_t st = ctx->stream;
  AggPartial *d_part = f.at<AggPartial>(aw.o_part), *d_out = f.at<AggPartial>(aw.o_back);
  if (const int rc = agg_upload(f, aw, insns, ops)) return rc;
  // (the expression kernel with the divide, or with the divide and the conditionals, only for a list that needs it)
  const bool div = agg_ops_hold_division(ops.data(), ops.size()), cond = agg_ops_hold_conditional(ops.data(), ops.size()), conv = agg_ops_hold_conversion(ops.data(), ops.size());
  if (const int rc = agg_launch_partials(f, aw, !ops.empty(), agg_partial_kernel, conv ? agg_expr_conv_partial_kernel : cond ? agg_expr_cond_partial_kernel : div ? agg_expr_div_partial_kernel : agg_expr_partial_kernel, rows, d_part)) return rc;
  hipLaunchKernelGGL(agg_final_kernel, dim3(aw.n_insn), dim3(256), 0, st, f.at<const AggInsn>(aw.o_insn), d_part, aw.blocks, d_out);
  HIP_TRY(ctx, hipGetLastError());
  // ---- the aggregation's one wait: a record per aggregate, and the kept row count ----
  HIP_TRY(ctx, hipMemcpyAsync(records, d_out, aw.back_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return ORCGPU_OK;
}

// The planes of the list's distinct conditions, behind the keep mask and in front of the partial kernels: the spans go up (where
// each condition's program lies in the call's predicate program, `first` instructions in), agg_cond_eval_kernel writes every word
// of every plane
int agg_run_conds(const FilterCall& f, const FilterWorkspace& ws, const AggWorkspace& aw, const orcgpu_host::AggPlan& aplan, uint32_t first, const KeptRows& rows) {
  std::vector<AggCondSpan> spans = aplan.cond_spans;
  for (AggCondSpan& sp : spans) sp.first += first;
  HIP_TRY(f.ctx, f.ctx->upload(f.X + aw.o_spans, spans.data(), spans.size() * sizeof(AggCondSpan), f.ctx->stream));
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((ws.n_words + 3) / 4, 16384);
  hipLaunchKernelGGL(agg_cond_eval_kernel, dim3(blocks, aw.n_conds), dim3(256), 0, f.ctx->stream, f.at<const FilterInsn>(ws.o_prog), (uint32_t)f.plan.prog.size(),
                     f.at<const AggCondSpan>(aw.o_spans), f.at<const uint8_t>(ws.o_lits), rows, f.at<const unsigned long long>(ws.o_planes),
                     f.at<unsigned long long>(aw.o_cond));
  HIP_TRY(f.ctx, hipGetLastError());
  return ORCGPU_OK;
}

// The key list as the kernels take it; ORCGPU_GROUP_HASH_BITS is read per call
GroupKeys group_keys_of(const orcgpu_host::GroupPlan& gplan) {
  GroupKeys keys{};
  keys.n = (uint32_t)gplan.keys.size();
  keys.hash_mask = orcgpu_host::group_hash_mask(getenv("ORCGPU_GROUP_HASH_BITS"));
  for (uint32_t k = 0; k < keys.n; k++) {
    keys.col[k] = gplan.keys[k].col;
    keys.fkind[k] = gplan.keys[k].fkind;
  }
  return keys;
}
// ORCGPU_POISON, the debugging aid of the decode, over the aggregation's tables of every path, in front of everything the call
// enqueues: nothing may depend on what the workspace held before.  (A failure to fill is not the call's failure.)
void agg_poison(const FilterCall& f, const AggWorkspace& gw) {
  static const char* poison = getenv("ORCGPU_POISON");
  if (poison && *poison) (void)hipMemsetAsync(f.X + gw.o_insn, (int)strtol(poison, nullptr, 0) & 0xFF, gw.bytes - gw.o_insn, f.ctx->stream);
}

// The grouped reduction behind the evaluation and its one wait: `set` gets the result's groups in first-appearance order, with
// the instructions' records and behind them the group's kept row count
int group_run(const FilterCall& f, const AggWorkspace& gw, const KeptRows& rows, const orcgpu_host::GroupPlan& gplan, const std::vector<AggInsn>& insns,
              const std::vector<AggExprOp>& ops, orcgpu_host::GroupSet& set) {
  orcgpu_ctx* ctx = f.ctx;
  hipStream_t st = ctx->stream;
  const GroupKeys keys = group_keys_of(gplan);
  GroupSlot* d_table = f.at<GroupSlot>(gw.o_table);
  GroupControl* d_ctl = f.at<GroupControl>(gw.o_back);
  uint32_t *d_plane = f.at<uint32_t>(gw.o_plane), *d_slot_group = f.at<uint32_t>(gw.o_slot_group);
  AggPartial *d_part = f.at<AggPartial>(gw.o_part), *d_out = f.at<AggPartial>(gw.o_back + gw.back_vals);
  if (const int rc = agg_upload(f, gw, insns, ops)) return rc;
  HIP_TRY(ctx, hipMemsetAsync(d_table, 0, gw.zero_bytes, st));
  HIP_TRY(ctx, hipMemsetAsync(d_ctl, 0, gw.back_bytes, st));
  hipLaunchKernelGGL(group_assign_kernel, dim3(gw.blocks), dim3(256), 0, st, keys, rows, d_table, d_ctl, d_plane);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(group_number_kernel, dim3(1), dim3(kGroupSlots), 0, st, keys, rows, d_table, d_ctl, d_slot_group, f.at<GroupKeyRecord>(gw.o_back + gw.back_keys));
  HIP_TRY(ctx, hipGetLastError());
  if (const int rc = agg_launch_partials(f, gw, !ops.empty(), agg_group_partial_kernel,
                                         agg_ops_hold_conversion(ops.data(), ops.size()) ? agg_group_expr_conv_partial_kernel
                                         : agg_ops_hold_conditional(ops.data(), ops.size()) ? agg_group_expr_cond_partial_kernel
                                         : agg_ops_hold_division(ops.data(), ops.size()) ? agg_group_expr_div_partial_kernel : agg_group_expr_partial_kernel, rows, (const uint32_t*)d_plane,
                                         (const uint32_t*)d_slot_group, (const GroupControl*)d_ctl, d_part))
    return rc;
  hipLaunchKernelGGL(agg_group_final_kernel, dim3(kGroupMax, gw.n_insn), dim3(256), 0, st, f.at<const AggInsn>(gw.o_insn), d_part, gw.blocks, d_ctl, d_out);
  HIP_TRY(ctx, hipGetLastError());
  // ---- the grouped aggregation's one wait: the group count and the flags, the key records, the value records ----
  std::vector<uint8_t> back(gw.back_bytes);
  HIP_TRY(ctx, hipMemcpyAsync(back.data(), d_ctl, gw.back_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  GroupControl ctl;
  memcpy(&ctl, back.data(), sizeof(ctl));
  char err[256];
  if (const int rc = orcgpu_host::group_check_flags(gplan, ctl.flags, ctl.n_groups, f.column_names, err, sizeof(err))) {
    set_err(ctx, "%s", err);
    return rc;
  }
  const uint32_t n = ctl.n_groups, nk = keys.n, ni = gw.n_insn;
  set.keys.resize((size_t)n * nk);
  set.vals.resize((size_t)n * ni);
  if (n) memcpy(set.keys.data(), back.data() + gw.back_keys, (size_t)n * nk * sizeof(GroupKeyRecord));
  const AggPartial* vals = reinterpret_cast<const AggPartial*>(back.data() + gw.back_vals);  // [instruction][kGroupMax]
  for (uint32_t g = 0; g < n; g++)
    for (uint32_t k = 0; k < ni; k++) set.vals[(size_t)g * ni + k] = vals[(size_t)k * kGroupMax + g];
  return ORCGPU_OK;
}

// group_run where the plan's limit is above kGroupMax: the same answer by the wide path, for whatever the rows hold
int group_run_wide(const FilterCall& f, const AggWorkspace& gw, const KeptRows& rows, const orcgpu_host::GroupPlan& gplan, const std::vector<AggInsn>& insns,
                   const std::vector<AggExprOp>& ops, orcgpu_host::GroupSet& set) {
  orcgpu_ctx* ctx = f.ctx;
  hipStream_t st = ctx->stream;
  const orcgpu_host::GroupWideLayout& w = gw.wide;
  if (f.n_in >= 0xffffffffull - 64) {  // (a pair of the sort holds its input row in 32 bits)
    set_err(ctx, "group by: a result of %llu input rows is more than a limit above ORCGPU_GROUP_MAX takes", (unsigned long long)f.n_in);
    return ORCGPU_UNSUPPORTED;
  }
  const GroupKeys keys = group_keys_of(gplan);
  const uint64_t n_in = f.n_in;
  GroupSlot* d_table = f.at<GroupSlot>(w.o_table);
  GroupControl* d_ctl = f.at<GroupControl>(w.o_ctl);
  uint32_t *d_plane = f.at<uint32_t>(w.o_plane), *d_slot_group = f.at<uint32_t>(w.o_slot_group), *d_first = f.at<uint32_t>(w.o_blk_first),
           *d_kept = f.at<uint32_t>(w.o_blk_kept), *d_hist = f.at<uint32_t>(w.o_hist), *d_seg = f.at<uint32_t>(w.o_seg);
  uint32_t *d_keys[2] = {f.at<uint32_t>(w.o_keys[0]), f.at<uint32_t>(w.o_keys[1])}, *d_rows[2] = {f.at<uint32_t>(w.o_rows[0]), f.at<uint32_t>(w.o_rows[1])};
  GroupKeyRecord* d_key_recs = f.at<GroupKeyRecord>(w.o_key_recs);
  AggPartial* d_vals = f.at<AggPartial>(w.o_vals);
  if (const int rc = agg_upload(f, gw, insns, ops)) return rc;
  HIP_TRY(ctx, hipMemsetAsync(d_table, 0, w.table_bytes, st));
  HIP_TRY(ctx, hipMemsetAsync(d_ctl, 0, sizeof(GroupControl), st));
  hipLaunchKernelGGL(group_wide_assign_kernel, dim3(gw.blocks), dim3(256), 0, st, keys, rows, d_table, w.slots, gplan.max_groups, d_ctl, d_plane);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(group_wide_count_kernel, dim3(w.tiles), dim3(256), 0, st, rows, (const GroupSlot*)d_table, w.slots, (const uint32_t*)d_plane, d_first, d_kept);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(group_wide_scan_kernel, dim3(1), dim3(1024), 0, st, d_first, w.tiles, &d_ctl->n_groups, gplan.max_groups, &d_ctl->flags);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(group_wide_scan_kernel, dim3(1), dim3(1024), 0, st, d_kept, w.tiles, &d_ctl->kept, 0u, &d_ctl->flags);
  HIP_TRY(ctx, hipGetLastError());
  hipLaunchKernelGGL(group_wide_number_kernel, dim3(w.tiles), dim3(256), 0, st, keys, rows, (const GroupSlot*)d_table, w.slots, w.cap, (const uint32_t*)d_plane,
                     (const uint32_t*)d_first, (const uint32_t*)d_kept, d_ctl, d_slot_group, d_key_recs, d_rows[0]);
  HIP_TRY(ctx, hipGetLastError());
  const uint32_t flat = (uint32_t)std::min<uint64_t>((n_in + 255) / 256, 4096);  // the grid of the kernels that stride over the pairs
  hipLaunchKernelGGL(group_wide_keys_kernel, dim3(flat), dim3(256), 0, st, (const uint32_t*)d_plane, (const uint32_t*)d_slot_group, w.slots, w.cap, n_in,
                     (const GroupControl*)d_ctl, (const uint32_t*)d_rows[0], d_keys[0]);
  HIP_TRY(ctx, hipGetLastError());
  uint32_t at = 0;  // which of the two buffers holds the pairs
  for (uint32_t pass = 0; pass < w.passes; pass++, at ^= 1) {
    const uint32_t shift = pass * kGroupRadixBits;
    hipLaunchKernelGGL(group_wide_hist_kernel, dim3(w.tiles), dim3(256), 0, st, (const uint32_t*)d_keys[at], shift, n_in, (const GroupControl*)d_ctl, d_hist);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(group_wide_scan_kernel, dim3(1), dim3(1024), 0, st, d_hist, w.tiles * 256u, (uint32_t*)nullptr, 0u, &d_ctl->flags);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(group_wide_scatter_kernel, dim3(w.tiles), dim3(256), 0, st, (const uint32_t*)d_keys[at], (const uint32_t*)d_rows[at], d_keys[at ^ 1],
                       d_rows[at ^ 1], shift, n_in, (const GroupControl*)d_ctl, (const uint32_t*)d_hist);
    HIP_TRY(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(group_wide_segments_kernel, dim3(flat), dim3(256), 0, st, (const uint32_t*)d_keys[at], w.cap, n_in, (const GroupControl*)d_ctl, d_seg);
  HIP_TRY(ctx, hipGetLastError());
  {
    // one wavefront a group, four a block: as many blocks as the records have room for groups, up to a grid that fills the device
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)w.cap + 3) / 4, 8192);
    const AggInsn* d_insn = f.at<const AggInsn>(gw.o_insn);
    hipLaunchKernelGGL(agg_group_wide_kernel, dim3(blocks, gw.n_insn), dim3(256), 0, st, d_insn, rows, (const uint32_t*)d_rows[at], (const uint32_t*)d_seg,
                       (const GroupControl*)d_ctl, w.cap, d_vals);
    HIP_TRY(ctx, hipGetLastError());
    if (!ops.empty()) {
      hipLaunchKernelGGL(agg_ops_hold_conversion(ops.data(), ops.size()) ? agg_group_wide_expr_conv_kernel : agg_ops_hold_conditional(ops.data(), ops.size()) ? agg_group_wide_expr_cond_kernel : agg_ops_hold_division(ops.data(), ops.size()) ? agg_group_wide_expr_div_kernel : agg_group_wide_expr_kernel, dim3(blocks, gw.n_insn), dim3(256), 0, st, d_insn, f.at<const AggExprOp>(gw.o_ops), rows, (const uint32_t*)d_rows[at],
                         (const uint32_t*)d_seg, (const GroupControl*)d_ctl, w.cap, d_vals);
      HIP_TRY(ctx, hipGetLastError());
    }
  }
  // ---- the first wait: the group count and the flags ----
  GroupControl ctl;
  HIP_TRY(ctx, hipMemcpyAsync(&ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  char err[256];
  if (const int rc = orcgpu_host::group_check_flags(gplan, ctl.flags, ctl.n_groups, f.column_names, err, sizeof(err))) {
    set_err(ctx, "%s", err);
    return rc;
  }
  if (ctl.n_groups > w.cap) {  // (more groups than input rows: nothing is sized by such a count)
    set_err(ctx, "group by: %u groups of %llu input rows", ctl.n_groups, (unsigned long long)n_in);
    return ORCGPU_UNEXPECTED;
  }
  // ---- the second: exactly n_groups key records and n_groups x instructions value records ----
  const uint32_t n = ctl.n_groups, nk = keys.n, ni = gw.n_insn;
  set.keys.resize((size_t)n * nk);
  set.vals.resize((size_t)n * ni);
  if (!n) return ORCGPU_OK;
  HIP_TRY(ctx, hipMemcpyAsync(set.keys.data(), d_key_recs, (size_t)n * nk * sizeof(GroupKeyRecord), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(set.vals.data(), d_vals, (size_t)n * ni * sizeof(AggPartial), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return ORCGPU_OK;
}

// The rows of `r` that `fplan` keeps (null: all of them), reduced by `aplan`.  Without a GROUP BY (gplan null) set.vals gets one
// record per instruction of the plan and behind them the kept row count (in w[0]), whatever the rows, and set.keys nothing; with
// one, `set` gets the groups of the kept rows, every group's records and behind them its kept row count.  *rows_kept: the kept
// rows, over the groups.  column_names: the result's columns, for the messages.
int result_aggregate_call(orcgpu_ctx* ctx, const orcgpu_result* r_, const orcgpu_host::FilterPlan* fplan, const orcgpu_host::AggPlan& aplan,
                          const orcgpu_host::GroupPlan* gplan, orcgpu_host::GroupSet& set, uint64_t* rows_seen, uint64_t* rows_kept,
                          const char* const* column_names, uint32_t n_names) {
  static const orcgpu_host::FilterPlan no_filter;
  orcgpu_result* r = const_cast<orcgpu_result*>(r_);  // (what is written is the filter's scratch allocation, never a batch)
  set = orcgpu_host::GroupSet{};
  set.n_keys = gplan ? (uint32_t)gplan->keys.size() : 0;
  set.n_insn = (uint32_t)aplan.insns.size() + 1;
  if (!gplan) set.vals.assign(set.n_insn, AggPartial{});
  if (rows_seen) *rows_seen = 0;
  if (rows_kept) *rows_kept = 0;
  if (r->status) return r->status;
  // the call's predicate program: the row filter's, and behind it the programs of the aggregates' conditions
  const size_t n_conds = aplan.cond_spans.size();
  const orcgpu_host::FilterPlan* const row_plan = fplan ? fplan : &no_filter;
  orcgpu_host::FilterPlan both;
  uint32_t cond_first = 0;
  if (n_conds) {
    if (fplan) both = *fplan;
    cond_first = orcgpu_host::filter_plan_append(both, aplan.conds);
  }
  const orcgpu_host::FilterPlan* const program = n_conds ? &both : row_plan;
  FilterCall f{ctx, r, *program, column_names, n_names, fplan != nullptr, fplan ? (uint32_t)fplan->prog.size() : 0u};
  if (const int rc = filter_open(f, rows_seen)) return rc;
  const FilterWorkspace ws = filter_workspace(f);
  const AggWorkspace aw(ws.bytes, (uint32_t)aplan.insns.size(), gplan, f.n_in, aplan.ops.size(), n_conds);
  if (const int rc = filter_reserve(f, ws, aw.bytes, gplan ? "the grouped aggregation" : "the aggregation")) return rc;
  std::vector<AggInsn> insns = aplan.insns;
  if (!orcgpu_host::agg_plan_in_bounds(insns, aplan.ops, f.nc, (uint32_t)n_conds) || !orcgpu_host::agg_conds_in_bounds(aplan.cond_spans, cond_first, f.plan.prog.size()))
    return ORCGPU_UNEXPECTED;
  if (gplan && !group_plan_in_bounds(*gplan, f)) return ORCGPU_UNEXPECTED;
  AggInsn kept{};
  kept.kind = AK_COUNT_ROWS;
  insns.push_back(kept);
  if (!f.n_in) return ORCGPU_OK;  // (no input row: every record is the empty one; no group)
  agg_poison(f, aw);
  if (const int rc = filter_upload(f, ws)) return rc;
  if (f.has_filter || n_conds)
    if (const int rc = filter_run_eval(f, ws)) return rc;
  KeptRows rows = filter_kept_rows(f, ws);
  if (n_conds) {
    if (const int rc = agg_run_conds(f, ws, aw, aplan, cond_first, rows)) return rc;
    rows.cond = f.at<const unsigned long long>(aw.o_cond);
    rows.n_cond = aw.n_conds;
  }
  if (const int rc = gplan ? (orcgpu_host::group_is_wide(gplan->max_groups) ? group_run_wide : group_run)(f, aw, rows, *gplan, insns, aplan.ops, set) : agg_run(f, aw, rows, insns, aplan.ops, set.vals.data())) return rc;
  uint64_t total = 0;  // the last record of every group: its kept rows
  for (size_t k = set.n_insn - 1; k < set.vals.size(); k += set.n_insn) total += set.vals[k].w[0];
  if (total > f.n_in) {
    set_err(ctx, "%s: %llu rows kept of %llu", gplan ? "group by" : "aggregate", (unsigned long long)total, (unsigned long long)f.n_in);
    return ORCGPU_UNEXPECTED;
  }
  if (rows_kept) *rows_kept = total;
  return ORCGPU_OK;
}

// What the two entry points check of their arguments alike (`what` opens the message)
int result_aggregate_args(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes, const char* const* column_names,
                          uint32_t n_columns, const void* out, const char* what) {
  if (!ctx || !r || (n_nodes && !nodes) || (n_columns && !column_names) || !out) return ORCGPU_INVALID_ARGUMENT;
  if (r->status) return r->status;
  if (n_columns != r->cols.size()) {
    set_err(ctx, "%s: %u column names for a result of %zu columns", what, n_columns, r->cols.size());
    return ORCGPU_INVALID_ARGUMENT;
  }
  return ORCGPU_OK;
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
  return orcgpu_result_aggregate_filters(ctx, r, nodes, n_nodes, column_names, n_columns, specs, exprs, nullptr, n_specs, out);
}
extern "C" int orcgpu_result_aggregate_filters(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                               const char* const* column_names, uint32_t n_columns, const orcgpu_agg_spec* specs,
                                               const orcgpu_agg_expr* exprs, const orcgpu_agg_filter* filters, uint32_t n_specs, orcgpu_agg_value* out) {
  if (const int rc = result_aggregate_args(ctx, r, nodes, n_nodes, column_names, n_columns, out, "aggregate")) return rc;
  orcgpu_host::AggPlan aplan;
  if (const int rc = result_compile_aggs(ctx, r, specs, exprs, filters, n_specs, column_names, aplan)) return rc;
  orcgpu_host::FilterPlan fplan;
  if (n_nodes)
    if (const int rc = result_compile_filter(ctx, r, nodes, n_nodes, column_names, fplan)) return rc;
  orcgpu_host::GroupSet set;
  if (const int rc = result_aggregate_call(ctx, r, n_nodes ? &fplan : nullptr, aplan, nullptr, set, nullptr, nullptr, column_names, n_columns)) return rc;
  for (uint32_t k = 0; k < n_specs; k++) orcgpu_host::agg_finish(aplan.insns[k], set.vals[k], &out[k]);
  return ORCGPU_OK;
}

extern "C" int orcgpu_result_aggregate_groups(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                              const char* const* column_names, uint32_t n_columns, const char* const* key_columns, uint32_t n_keys,
                                              const orcgpu_agg_spec* specs, uint32_t n_specs, orcgpu_groups** out) {
  return orcgpu_result_aggregate_groups_limit(ctx, r, nodes, n_nodes, column_names, n_columns, key_columns, n_keys, specs, nullptr, n_specs, 0, out);
}
extern "C" int orcgpu_result_aggregate_groups_exprs(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                                    const char* const* column_names, uint32_t n_columns, const char* const* key_columns, uint32_t n_keys,
                                                    const orcgpu_agg_spec* specs, const orcgpu_agg_expr* exprs, uint32_t n_specs, orcgpu_groups** out) {
  return orcgpu_result_aggregate_groups_limit(ctx, r, nodes, n_nodes, column_names, n_columns, key_columns, n_keys, specs, exprs, n_specs, 0, out);
}
extern "C" int orcgpu_result_aggregate_groups_limit(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                                    const char* const* column_names, uint32_t n_columns, const char* const* key_columns, uint32_t n_keys,
                                                    const orcgpu_agg_spec* specs, const orcgpu_agg_expr* exprs, uint32_t n_specs, uint32_t max_groups,
                                                    orcgpu_groups** out) {
  return orcgpu_result_aggregate_groups_filters(ctx, r, nodes, n_nodes, column_names, n_columns, key_columns, n_keys, specs, exprs, nullptr, n_specs, max_groups, out);
}
extern "C" int orcgpu_result_aggregate_groups_filters(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                                      const char* const* column_names, uint32_t n_columns, const char* const* key_columns, uint32_t n_keys,
                                                      const orcgpu_agg_spec* specs, const orcgpu_agg_expr* exprs, const orcgpu_agg_filter* filters,
                                                      uint32_t n_specs, uint32_t max_groups, orcgpu_groups** out) {
  if (out) *out = nullptr;
  if (const int rc = result_aggregate_args(ctx, r, nodes, n_nodes, column_names, n_columns, out, "group by")) return rc;
  orcgpu_host::GroupPlan gplan;
  if (const int rc = result_compile_group(ctx, r, key_columns, n_keys, column_names, gplan)) return rc;
  {
    char err[256];
    uint32_t total = 0;  // (one result: the total over stripes is not this call's; the highest keeps it out of the way)
    if (const int rc = orcgpu_host::group_limits(max_groups, ORCGPU_GROUP_TOTAL_LIMIT_MAX, &gplan.max_groups, &total, err, sizeof(err))) {
      set_err(ctx, "%s", err);
      return rc;
    }
  }
  orcgpu_host::AggPlan aplan;
  if (const int rc = result_compile_aggs(ctx, r, specs, exprs, filters, n_specs, column_names, aplan)) return rc;
  orcgpu_host::FilterPlan fplan;
  if (n_nodes)
    if (const int rc = result_compile_filter(ctx, r, nodes, n_nodes, column_names, fplan)) return rc;
  orcgpu_host::GroupSet set;
  if (const int rc = result_aggregate_call(ctx, r, n_nodes ? &fplan : nullptr, aplan, &gplan, set, nullptr, nullptr, column_names, n_columns)) return rc;
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
