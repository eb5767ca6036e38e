// orcgpu_filter.inc -- the row filter at the seam: orcgpu_result_filter and what the file reader calls per stripe.  The plan
// compiler is orcgpu_filter_plan.inc (host only), the call's arithmetic orcgpu_filter_host.inc (host only), the kernels
// device/filter_kernels.hip; what is left here touches the device.
//
// One filtered result costs ONE host wait: behind evaluate -> scan -> place -> count the host fetches the kept row count with
// the per-batch null counts and string byte totals (filter_run_front, "the filter's one wait"); with them it lays the
// output arena out compactly -- so that a copy back moves the kept rows' bytes and no more -- and enqueues the gather, which
// nobody waits for: orcgpu_result_fetch_async orders its copies behind the decode stream.
//
// The aggregation's calls (orcgpu_agg.inc) open the way the filter's does and evaluate with its kernels: the opening
// (filter_open, filter_workspace, filter_reserve), the predicate's compile against a result (result_compile_filter) and the
// kernel argument for the rows (filter_kept_rows) stand here once, for the three of them.
#include "orcgpu_filter_host.inc"
namespace {

static_assert(kFilterAlign == kAlign && kFilterColBytes == sizeof(FilterCol) && kFilterJobBytes == sizeof(FilterGatherJob) && kFilterSegBytes == sizeof(SelBatch),
              "orcgpu_filter_host.inc states the alignment and the sizes of the device's structs");

int enc_scan(orcgpu_ctx* ctx, hipStream_t st, const uint32_t* d_in, uint64_t count, uint64_t* d_sums, uint64_t* d_total, uint64_t* d_out);

// One call on a decoded result -- the row filter's, or an aggregation's (orcgpu_agg.inc), which borrows the front of the filter's
// pipeline up to the evaluation: what its steps hand on
struct FilterCall {
  orcgpu_ctx* ctx;
  orcgpu_result* r;
  const orcgpu_host::FilterPlan& plan;
  const char* const* column_names;  // the result's columns, for the messages (null: none)
  uint32_t n_names;
  bool has_filter = true;  // false: an aggregation without a predicate -- `plan` holds no row filter, no keep mask is evaluated
  // the row filter's instructions in front of plan.prog (~0: all of it).  An aggregation whose aggregates carry conditions lays
  // their programs behind them (filter_plan_append): the plane kernels serve the whole program, filter_eval_kernel runs this front
  uint32_t n_row_insn = ~0u;
  uint32_t nc = 0, B = 0, W = 0, src_batches = 0;  // (src_batches: uniform batches of the decode)
  std::vector<SelBatch> segs;       // the input rows: those of a row selection's batches (none: the stripe's) ...
  std::vector<uint64_t> seg_first;  // ... and the input row each starts at
  uint64_t n_in = 0;
  std::vector<FilterColDesc> descs;
  std::vector<FilterCol> fcols;
  uint8_t* X = nullptr;       // the workspace on the device
  std::vector<uint8_t> host;  // the first upload
  template <typename T>
  T* at(uint64_t off) const { return reinterpret_cast<T*>(X + off); }
};

int filter_refuse(orcgpu_ctx* ctx, const orcgpu_result* r) {
  if (r->hold && orcgpu_hold::hold_exported(r->hold)) {
    set_err(ctx, "a result that exported device batches still view cannot be filtered");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (r->filtered) {
    set_err(ctx, "a row filter has already been applied to this result");
    return ORCGPU_INVALID_ARGUMENT;
  }
  for (const ColumnOut& co : r->cols) {
    if (co.is_struct || co.is_union || co.is_list || co.elem || co.parent >= 0 || !r->subs.empty()) {
      set_err(ctx, "row filter: column %u of the result is nested (Struct / List / Map / Union are not filtered)", co.column_id);
      return ORCGPU_UNSUPPORTED;
    }
    if (!co.is_bool && !co.is_string && co.width != 1 && co.width != 2 && co.width != 4 && co.width != 8 && co.width != 16) {
      set_err(ctx, "row filter: column %u has values of %u bytes", co.column_id, co.width);
      return ORCGPU_UNSUPPORTED;
    }
  }
  return ORCGPU_OK;
}

void filter_segments(FilterCall& f) {
  f.n_in = f.r->n_rows;
  if (!f.r->selected) return;
  f.n_in = 0;
  for (auto& b : f.r->sel) {
    f.seg_first.push_back(f.n_in);
    f.segs.push_back(b);
    f.n_in += b.len;
  }
}

FilterColDesc filter_desc_of(const ColumnOut& co) {  // (in the order FilterColDesc declares them)
  return {co.orc_type, co.width, co.ts_unit, co.is_bool, co.is_string, co.has_present, co.dict_out, co.dict_decoded, co.dict_len, co.dict_bytes};
}
void filter_describe(FilterCall& f) {
  for (const ColumnOut& co : f.r->cols) f.descs.push_back(filter_desc_of(co));
}

// The columns as the kernels see them, with pointers into the decode's arenas; the char bases of the string columns go into the
// first upload
void filter_fill_cols(FilterCall& f, const FilterWorkspace& ws) {
  uint8_t* const host = f.host.data();
  f.fcols.resize(f.nc);
  for (uint32_t c = 0; c < f.nc; c++) {
    const ColumnOut& co = f.r->cols[c];
    const uint8_t* A = f.r->filtered ? f.r->filt_arena.p : f.r->arena[co.lane].p;  // (a filtered result, aggregated: the kept rows' arena)
    FilterCol& fc = f.fcols[c];
    memset(&fc, 0, sizeof(fc));
    bool has_validity = co.has_present && f.r->n_rows;
    if (f.r->filtered) {  // (the kept rows carry a validity buffer only when one of them is null)
      has_validity = false;
      for (const uint64_t n : co.null_counts) has_validity = has_validity || n;
    }
    fc.validity = has_validity ? reinterpret_cast<const unsigned long long*>(A + co.validity_off) : nullptr;
    fc.width = co.width;
    fc.kind = filter_col_kind(f.descs[c]);
    if (co.is_string) {
      fc.offsets = reinterpret_cast<const int32_t*>(A + co.offsets_off);
      fc.chars = (co.values_in_chars ? f.r->chars[co.lane].p : A) + co.values_off;
      fc.char_base = f.at<const unsigned long long>(ws.o_cbase[c]);
      for (size_t k = 0; k < co.char_base.size() && k < f.src_batches; k++) reinterpret_cast<uint64_t*>(host + ws.o_cbase[c])[k] = co.char_base[k];
    } else fc.values = A + co.values_off;
  }
}

int filter_check(FilterCall& f) {
  const char* const* column_names = f.column_names;
  const uint32_t n_names = f.n_names;
  std::vector<uint32_t> kinds(f.nc);
  for (uint32_t c = 0; c < f.nc; c++) kinds[c] = f.fcols[c].kind;
  uint32_t col = 0;
  const int rc = filter_check_kinds(f.plan, kinds.data(), f.descs.data(), f.nc, &col);
  if (rc == ORCGPU_UNSUPPORTED) {
    char err[256];
    filter_dict_refusal(err, sizeof(err), column_names && col < n_names ? column_names[col] : nullptr, f.r->cols[col].column_id);
    set_err(f.ctx, "%s", err);
  } else if (rc) set_err(f.ctx, "row filter: column %u is not decoded to the type its comparison needs", col < f.nc ? f.r->cols[col].column_id : col);
  return rc;
}

// The first upload: the program, its literals and leaf lists, the segments and the columns (nothing goes up for no input row)
int filter_upload(FilterCall& f, const FilterWorkspace& ws) {
  orcgpu_ctx* ctx = f.ctx;
  std::vector<uint8_t>& host = f.host;
  hipStream_t st = ctx->stream;
  const orcgpu_host::FilterPlan& plan = f.plan;
  const uint32_t n_segs = (uint32_t)f.segs.size(), n_insn = (uint32_t)plan.prog.size(), n_like = (uint32_t)plan.like_leaves.size(), n_set = (uint32_t)plan.in_leaves.size();
  const uint32_t n_expr = (uint32_t)plan.expr_leaves.size();
  if (n_insn) memcpy(host.data() + ws.o_prog, plan.prog.data(), n_insn * sizeof(FilterInsn));
  if (!plan.lits.empty()) memcpy(host.data() + ws.o_lits, plan.lits.data(), plan.lits.size());
  if (n_like) memcpy(host.data() + ws.o_leaves, plan.like_leaves.data(), (size_t)n_like * 4);
  if (n_set) memcpy(host.data() + ws.o_leaves + (size_t)n_like * 4, plan.in_leaves.data(), (size_t)n_set * 4);
  if (n_expr) memcpy(host.data() + ws.o_leaves + ((size_t)n_like + n_set) * 4, plan.expr_leaves.data(), (size_t)n_expr * 4);
  if (n_segs) {
    memcpy(host.data() + ws.o_segs, f.segs.data(), (size_t)n_segs * sizeof(SelBatch));
    memcpy(host.data() + ws.o_first, f.seg_first.data(), (size_t)n_segs * 8);
  }
  if (f.nc) memcpy(host.data() + ws.o_cols, f.fcols.data(), (size_t)f.nc * sizeof(FilterCol));
  if (!f.n_in) return ORCGPU_OK;
  HIP_TRY(ctx, ctx->upload(f.X, host.data(), ws.up_bytes, st));
  HIP_TRY(ctx, hipMemsetAsync(f.at<unsigned long long>(ws.o_counters), 0, (ws.n_counters + 1) * 8, st));  // (+ 1: the overflow count)
  return ORCGPU_OK;
}

// Plane kernels -> evaluate: the keep mask (one word per 64 input rows) and its popcounts, and nothing after them -- what the
// filter compacts from and the aggregation reduces from.  (No row filter -- an aggregation with conditions only: the plane kernels
// alone.)
int filter_run_eval(FilterCall& f, const FilterWorkspace& ws) {
  orcgpu_ctx* ctx = f.ctx;
  hipStream_t st = ctx->stream;
  const orcgpu_host::FilterPlan& plan = f.plan;
  const uint32_t n_segs = (uint32_t)f.segs.size(), n_insn = (uint32_t)plan.prog.size(), n_like = (uint32_t)plan.like_leaves.size(), n_set = (uint32_t)plan.in_leaves.size();
  const FilterInsn* d_prog = f.at<const FilterInsn>(ws.o_prog);
  const uint8_t* d_lits = f.at<const uint8_t>(ws.o_lits);
  const uint32_t* d_leaves = f.at<const uint32_t>(ws.o_leaves);
  const FilterCol* d_cols = f.at<const FilterCol>(ws.o_cols);
  const SelBatch* d_segs = f.at<const SelBatch>(ws.o_segs);
  const unsigned long long* d_first = f.at<const unsigned long long>(ws.o_first);
  unsigned long long *d_keep = f.at<unsigned long long>(ws.o_keep), *d_planes = f.at<unsigned long long>(ws.o_planes);
  const uint32_t n_expr = (uint32_t)plan.expr_leaves.size(), n_planes = (uint32_t)plan.n_planes();
  const uint32_t eval_blocks = (uint32_t)std::min<uint64_t>((ws.n_words + 3) / 4, 16384);
  if (n_like) {  // the matcher first: the evaluation reads its bits
    hipLaunchKernelGGL(filter_like_kernel, dim3(eval_blocks, n_like), dim3(256), 0, st, d_prog, n_insn, d_leaves, d_lits, d_cols, d_segs, d_first, n_segs, f.n_in, f.B, f.W,
                       d_planes, n_planes);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (n_set) {  // ... and the set membership of the IN leaves
    hipLaunchKernelGGL(filter_in_kernel, dim3(eval_blocks, n_set), dim3(256), 0, st, d_prog, n_insn, d_leaves + n_like, d_lits, d_cols, d_segs, d_first, n_segs, f.n_in, f.B, f.W,
                       d_planes, n_planes);
    HIP_TRY(ctx, hipGetLastError());
  }
  if (n_expr) {  // ... and the two sides of the expression leaves, compared: a T and an F plane each
    hipLaunchKernelGGL(orcgpu_host::filter_plan_holds_conversion(plan) ? filter_expr_conv_kernel : orcgpu_host::filter_plan_holds_conditional(plan) ? filter_expr_cond_kernel : orcgpu_host::filter_plan_holds_division(plan) ? filter_expr_div_kernel : filter_expr_kernel, dim3(eval_blocks, n_expr), dim3(256), 0, st, d_prog, n_insn, d_leaves + n_like + n_set, d_lits, d_cols, d_segs, d_first, n_segs, f.n_in,
                       f.B, f.W, d_planes, n_planes, f.at<unsigned long long>(ws.o_overflow));
    HIP_TRY(ctx, hipGetLastError());
  }
  if (!f.has_filter) return ORCGPU_OK;
  hipLaunchKernelGGL(filter_eval_kernel, dim3(eval_blocks), dim3(256), 0, st, d_prog, std::min(n_insn, f.n_row_insn), d_lits, d_cols, d_segs, d_first, n_segs, f.n_in, f.B,
                     f.W, d_keep, f.at<uint32_t>(ws.o_cnt), d_planes);
  HIP_TRY(ctx, hipGetLastError());
  return ORCGPU_OK;
}

// The first upload, then plane kernels -> evaluate -> scan -> place -> count, and the filter's one wait: `back` gets the kept
// row count, then null counts and string bytes per (column, output batch)
int filter_run_front(FilterCall& f, const FilterWorkspace& ws, std::vector<uint64_t>& back) {
  orcgpu_ctx* ctx = f.ctx;
  hipStream_t st = ctx->stream;
  if (const int rc = filter_upload(f, ws)) return rc;
  if (!f.n_in) return ORCGPU_OK;
  if (const int rc = filter_run_eval(f, ws)) return rc;
  const uint32_t n_segs = (uint32_t)f.segs.size(), nb_max = (uint32_t)ws.nb_max;
  const FilterCol* d_cols = f.at<const FilterCol>(ws.o_cols);
  const SelBatch* d_segs = f.at<const SelBatch>(ws.o_segs);
  const unsigned long long* d_first = f.at<const unsigned long long>(ws.o_first);
  unsigned long long *d_counters = f.at<unsigned long long>(ws.o_counters), *d_keep = f.at<unsigned long long>(ws.o_keep);
  uint32_t* d_rows = f.at<uint32_t>(ws.o_rows);
  const int rc = enc_scan(ctx, st, f.at<const uint32_t>(ws.o_cnt), ws.n_words, f.at<uint64_t>(ws.o_sums), reinterpret_cast<uint64_t*>(d_counters), f.at<uint64_t>(ws.o_woff));
  if (rc) return rc;
  hipLaunchKernelGGL(filter_place_kernel, dim3((uint32_t)((f.n_in + 255) / 256)), dim3(256), 0, st, d_keep, f.at<const unsigned long long>(ws.o_woff), d_segs, d_first, n_segs,
                     f.n_in, d_rows);
  HIP_TRY(ctx, hipGetLastError());
  for (uint32_t o = 0; o < f.nc; o += 65535u)
    hipLaunchKernelGGL(filter_count_kernel, dim3(nb_max, std::min<uint32_t>(65535u, f.nc - o)), dim3(256), 0, st, d_cols + o, d_rows, d_counters, f.B, f.W, nb_max,
                       d_counters + 1 + (uint64_t)o * nb_max, d_counters + 1 + ((uint64_t)f.nc + o) * nb_max);
  HIP_TRY(ctx, hipGetLastError());
  // ---- the filter's one wait: the kept row count, null counts and string bytes per output batch ----
  HIP_TRY(ctx, hipMemcpyAsync(back.data(), d_counters, (ws.n_counters + 1) * 8, hipMemcpyDeviceToHost, st));  // (the overflow count behind them)
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return ORCGPU_OK;
}

// The kept rows into the output arena as `out` places them: the dictionaries that go along, the second upload, the gather
int filter_run_gather(FilterCall& f, const FilterWorkspace& ws, const FilterOutput& out, uint64_t kept) {
  orcgpu_ctx* ctx = f.ctx;
  orcgpu_result* r = f.r;
  hipStream_t st = ctx->stream;
  if (!r->filt_arena.ensure(out.arena_bytes + kAlign)) {
    set_err(ctx, "hipMalloc(%llu) for the filtered rows failed", (unsigned long long)out.arena_bytes);
    return ORCGPU_HIP_ERROR;
  }
  uint8_t* O = r->filt_arena.p;
  std::vector<uint8_t> up2(ws.up2_bytes, 0);
  FilterGatherJob* jobs = reinterpret_cast<FilterGatherJob*>(up2.data());
  for (uint32_t c = 0; c < f.nc; c++) {
    FilterGatherJob& j = jobs[c];
    const FilterPlace& p = out.place[c];
    j.src = f.fcols[c];
    j.out_validity = p.has_validity ? reinterpret_cast<unsigned long long*>(O + p.validity) : nullptr;
    j.out_values = O + p.values;
    j.out_chars = O + p.values;
    j.out_offsets = reinterpret_cast<int32_t*>(O + p.offsets);
    j.out_char_base = f.at<const unsigned long long>(ws.o_obase) + (uint64_t)c * ws.nb_max;
    const ColumnOut& co = r->cols[c];
    if (!co.dict_out || !co.dict_decoded) continue;
    const uint8_t* A = r->arena[co.lane].p;
    HIP_TRY(ctx, hipMemcpyAsync(O + p.dict_offsets, A + co.dict_offsets_off, (co.dict_len + 1) * 4, hipMemcpyDeviceToDevice, st));
    if (co.dict_bytes) HIP_TRY(ctx, hipMemcpyAsync(O + p.dict_values, A + co.dict_values_off, co.dict_bytes, hipMemcpyDeviceToDevice, st));
  }
  if (!out.obase.empty()) memcpy(up2.data() + (ws.o_obase - ws.o_jobs), out.obase.data(), out.obase.size() * 8);
  HIP_TRY(ctx, ctx->upload(f.X + ws.o_jobs, up2.data(), up2.size(), st));
  for (uint32_t o = 0; o < f.nc; o += 65535u)
    hipLaunchKernelGGL(filter_gather_kernel, dim3(out.nbo, std::min<uint32_t>(65535u, f.nc - o)), dim3(256), 0, st, f.at<const FilterGatherJob>(ws.o_jobs) + o,
                       f.at<const uint32_t>(ws.o_rows), kept, f.B, f.W);
  HIP_TRY(ctx, hipGetLastError());
  return ORCGPU_OK;
}

// The result now speaks in the kept rows: uniform batches in the filter's own arena
void filter_adopt_output(orcgpu_result* r, FilterOutput& out, uint64_t kept) {
  for (size_t c = 0; c < r->cols.size(); c++) {
    ColumnOut& co = r->cols[c];
    FilterPlace& p = out.place[c];
    co.lane = 0;
    co.values_in_chars = false;
    co.validity_off = p.validity;
    co.values_off = p.values;
    co.offsets_off = p.offsets;
    if (co.dict_out) {
      if (!p.dict_kept) co.dict_len = co.dict_bytes = 0, co.dict_decoded = false;  // (no batch is left to refer to it)
      co.dict_offsets_off = p.dict_kept ? p.dict_offsets : 0;
      co.dict_values_off = p.dict_kept ? p.dict_values : 0;
    }
    co.null_counts = std::move(p.null_counts);
    co.char_base = std::move(p.char_base);
    co.char_total = std::move(p.char_total);
    co.sel_nulls.clear();
    co.sel_char_start.clear();
    co.sel_char_total.clear();
  }
  r->arrow_bytes = out.arrow_bytes;
  r->n_rows = kept;
  r->n_batches = out.nbo;
  r->selected = false;
  r->sel.clear();
  r->filtered = true;
  r->mirror_valid = false;
  r->dev_ready_recorded = false;
  if (out.status) {
    r->status = out.status;
    r->err_batch = out.err_batch;
    r->err_col = out.err_col;
  }
}

// The opening of a call on a decoded result, in two steps; between them a caller lays its own tables out behind ws.bytes.
// filter_open: the device, the input rows and what the columns are (*rows_seen: the input rows)
int filter_open(FilterCall& f, uint64_t* rows_seen) {
  HIP_TRY(f.ctx, hipSetDevice(f.ctx->device));
  f.nc = (uint32_t)f.r->cols.size();
  f.B = f.r->batch;
  f.W = f.r->words_per_batch;
  filter_segments(f);
  filter_describe(f);
  f.src_batches = f.r->selected ? f.r->full_batches : f.r->n_batches;
  if (rows_seen) *rows_seen = f.n_in;
  return ORCGPU_OK;
}
FilterWorkspace filter_workspace(const FilterCall& f, uint64_t out_rows_max = ~0ull) {
  return FilterWorkspace(f.plan, f.descs.data(), f.nc, (uint32_t)f.segs.size(), f.src_batches, f.n_in, f.B, out_rows_max);
}
// filter_reserve: `bytes` of workspace on the device (ws.bytes and what the caller laid behind it; `what` names the caller in
// the message), the columns into the first upload, and the plan against what the columns were decoded to
int filter_reserve(FilterCall& f, const FilterWorkspace& ws, uint64_t bytes, const char* what) {
  if (!f.r->filt_tmp.ensure(bytes + kAlign)) {
    set_err(f.ctx, "hipMalloc(%llu) for %s failed", (unsigned long long)bytes, what);
    return ORCGPU_HIP_ERROR;
  }
  f.X = f.r->filt_tmp.p;
  f.host.assign(ws.up_bytes, 0);
  filter_fill_cols(f, ws);
  return f.plan.prog.empty() ? ORCGPU_OK : filter_check(f);
}

// The rows an aggregation's kernels walk: the kernel argument, once per call
KeptRows filter_kept_rows(const FilterCall& f, const FilterWorkspace& ws) {
  return {f.at<const FilterCol>(ws.o_cols), f.at<const SelBatch>(ws.o_segs), f.at<const unsigned long long>(ws.o_first), (uint32_t)f.segs.size(), f.n_in, f.B, f.W,
          f.has_filter ? f.at<const unsigned long long>(ws.o_keep) : nullptr};
}

// The predicate's plan against a decoded result's columns (column_names: one per column of the result)
int result_compile_filter(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes, const char* const* column_names,
                          orcgpu_host::FilterPlan& plan) {
  const uint32_t n_columns = (uint32_t)r->cols.size();
  std::vector<int32_t> kinds(n_columns), params(n_columns, 0);
  for (uint32_t c = 0; c < n_columns; c++) {
    const ColumnOut& co = r->cols[c];
    kinds[c] = co.orc_type;
    params[c] = co.orc_type == ORCGPU_T_DECIMAL ? (int32_t)co.scale : co.ts_unit;  // what Decimal128 / TimestampNs literals are brought to
  }
  const orcgpu_host::KeySetRefs sets = ctx_key_set_refs(ctx);  // (what a set leaf may name)
  const int rc = orcgpu_host::filter_compile(nodes, n_nodes, column_names, kinds.data(), n_columns, plan, params.data(), &sets);
  if (rc) set_err(ctx, "%s", plan.err);
  return rc;
}

// Open, front, place, gather, adopt
int result_filter_plan(orcgpu_ctx* ctx, orcgpu_result* r, const orcgpu_host::FilterPlan& plan, uint64_t* rows_seen, uint64_t* rows_kept,
                       const char* const* column_names = nullptr, uint32_t n_names = 0, uint64_t* overflow_rows = nullptr) {
  if (rows_seen) *rows_seen = 0;
  if (overflow_rows) *overflow_rows = 0;
  if (rows_kept) *rows_kept = 0;
  if (r->status) return r->status;  // a failed decode is left as it is
  if (const int rc = filter_refuse(ctx, r)) return rc;
  FilterCall f{ctx, r, plan, column_names, n_names};
  if (const int rc = filter_open(f, rows_seen)) return rc;
  const FilterWorkspace ws = filter_workspace(f);
  if (const int rc = filter_reserve(f, ws, ws.bytes, "the row filter")) return rc;
  std::vector<uint64_t> back(ws.n_counters + 1, 0);
  if (const int rc = filter_run_front(f, ws, back)) return rc;
  const uint64_t kept = back[0];
  if (overflow_rows) *overflow_rows = back[ws.n_counters];
  if (kept > f.n_in) {
    set_err(ctx, "row filter: %llu rows kept of %llu", (unsigned long long)kept, (unsigned long long)f.n_in);
    return ORCGPU_UNEXPECTED;
  }
  FilterOutput out = filter_place_output(f.descs.data(), back.data(), f.nc, ws.nb_max, kept, f.B, f.W);
  r->filt_used = kept ? out.arena_bytes : 0;
  if (kept)
    if (const int rc = filter_run_gather(f, ws, out, kept)) return rc;
  filter_adopt_output(r, out, kept);
  if (rows_kept) *rows_kept = kept;
  return ORCGPU_OK;
}

}  // namespace

extern "C" int orcgpu_result_filter(orcgpu_ctx* ctx, orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes,
                                    const char* const* column_names, uint32_t n_columns, uint64_t* rows_kept) {
  if (!ctx || !r || !nodes || !n_nodes || (n_columns && !column_names)) return ORCGPU_INVALID_ARGUMENT;
  if (rows_kept) *rows_kept = 0;
  if (r->status) return r->status;
  if (n_columns != r->cols.size()) {
    set_err(ctx, "row filter: %u column names for a result of %zu columns", n_columns, r->cols.size());
    return ORCGPU_INVALID_ARGUMENT;
  }
  orcgpu_host::FilterPlan plan;
  if (const int rc = result_compile_filter(ctx, r, nodes, n_nodes, column_names, plan)) return rc;
  return result_filter_plan(ctx, r, plan, nullptr, rows_kept, column_names, n_columns);
}
