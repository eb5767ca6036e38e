// orcgpu_top_k.inc -- ORDER BY ... LIMIT k at the seam: orcgpu_result_top_k and what the file reader calls per stripe.  The plan
// compiler, the pass plan, the workspace and the key records' merge are orcgpu_top_k_host.inc (host only), the kernels
// device/top_k_kernels.hip; the filter's call (orcgpu_filter.inc) lends its FilterCall, its workspace, its opening, its evaluation
// and everything behind the row list: count, the ONE wait, gather, adoption.
//
//   open -> reserve (the selection's tables lie behind the filter's: TopKWorkspace) -> upload -> LIKE / IN planes, filter_eval_kernel
//   (no predicate: nothing is evaluated, every input row is a candidate) -> top_k_select: init, then per byte of the key string
//   pass + choose, the tail pass, tie count, enc_scan, final -> enc_scan, filter_place_kernel: the winners in ascending input order
//   -> top_k_sort: per byte, backwards, hist + scan + scatter -> top_k_records_kernel -> filter_count_kernel -> the wait, which
//   fetches the filter's counters, the select's state and min(k, n_in) key records -> filter_place_output, gather, adopt.
// The launch sequence is a function of the key kinds and k (grids: of the input row count too), never of the data.
#include "orcgpu_top_k_host.inc"
namespace {

// Do the keys read what is there?  A column of the result, decoded to the kind the key was planned for
bool top_k_plan_in_bounds(const orcgpu_host::TopKPlan& plan, const FilterCall& f) {
  const TopKKeys& keys = plan.keys;
  if (!keys.n || keys.n > kTopKMaxKeys || !keys.len || keys.len > kTopKMaxLen || !plan.k || plan.k > kTopKMax) return false;
  uint32_t at = 0;
  for (uint32_t q = 0; q < keys.n; q++) {
    const TopKKey& k = keys.key[q];
    if (k.col >= f.nc || f.fcols[k.col].kind != orcgpu_host::top_k_fkind(k) || f.descs[k.col].dict_out) return false;
    if (k.first != at || k.bytes != (k.kind == TK_DEC128 ? 17u : 9u)) return false;
    at += k.bytes;
  }
  return at == keys.len;
}

// The rows of the stripe the row list may name: all of it, or what the selection's batches reach
uint64_t top_k_source_rows(const FilterCall& f) {
  if (!f.r->selected) return f.r->n_rows;
  uint64_t n = 0;
  for (const SelBatch& b : f.segs) n = std::max<uint64_t>(n, b.start + b.len);
  return n;
}

// The radix select: cand / win -> the winners' plane and its popcounts (ws.o_cnt), from which the filter's scan and place go on
int top_k_select(const FilterCall& f, const FilterWorkspace& ws, const orcgpu_host::TopKWorkspace& tw, const orcgpu_host::TopKPlan& plan, const KeptRows& rows) {
  orcgpu_ctx* ctx = f.ctx;
  hipStream_t st = ctx->stream;
  const TopKKeys& keys = plan.keys;
  unsigned long long *d_cand = f.at<unsigned long long>(tw.o_cand), *d_win = f.at<unsigned long long>(tw.o_win), *d_final = f.at<unsigned long long>(tw.o_final);
  TopKState* d_state = f.at<TopKState>(tw.o_state);
  uint32_t* d_hist = f.at<uint32_t>(tw.o_hist);
  const uint32_t word_blocks = (uint32_t)((tw.n_words + 255) / 256);
  HIP_TRY(ctx, hipMemsetAsync(d_state, 0, tw.zero_bytes, st));
  hipLaunchKernelGGL(top_k_init_kernel, dim3(word_blocks), dim3(256), 0, st, rows.keep, f.n_in, plan.k, d_cand, d_win, d_state);
  HIP_TRY(ctx, hipGetLastError());
  const std::vector<orcgpu_host::TopKPass> passes = orcgpu_host::top_k_select_passes(keys);
  const uint32_t n_pass = (uint32_t)passes.size();
  for (uint32_t p = 0; p <= n_pass; p++) {  // (p = n_pass: the tail, which applies the last bin and counts nothing)
    const orcgpu_host::TopKPass prev = passes[p ? p - 1 : 0], cur = passes[p < n_pass ? p : n_pass - 1];
    hipLaunchKernelGGL(top_k_pass_kernel, dim3(tw.sel_blocks), dim3(256), 0, st, keys.key[prev.key], prev.byte, keys.key[cur.key], cur.byte, p, n_pass, rows, d_cand, d_win,
                       (const TopKState*)d_state, d_hist);
    HIP_TRY(ctx, hipGetLastError());
    if (p == n_pass) break;
    hipLaunchKernelGGL(top_k_choose_kernel, dim3(1), dim3(256), 0, st, p, tw.sel_blocks, (const uint32_t*)d_hist, d_state);
    HIP_TRY(ctx, hipGetLastError());
  }
  // the rows still tied on the whole key: in ascending row order up to the remainder
  hipLaunchKernelGGL(top_k_tie_count_kernel, dim3(word_blocks), dim3(256), 0, st, (const unsigned long long*)d_cand, tw.n_words, f.at<uint32_t>(tw.o_tie_cnt));
  HIP_TRY(ctx, hipGetLastError());
  if (const int rc = enc_scan(ctx, st, f.at<const uint32_t>(tw.o_tie_cnt), tw.n_words, f.at<uint64_t>(tw.o_tie_sums), f.at<uint64_t>(tw.o_tie_total), f.at<uint64_t>(tw.o_tie_off)))
    return rc;
  hipLaunchKernelGGL(top_k_final_kernel, dim3(word_blocks), dim3(256), 0, st, (const unsigned long long*)d_cand, (const unsigned long long*)d_win,
                     f.at<const unsigned long long>(tw.o_tie_off), (const TopKState*)d_state, tw.n_words, d_final, f.at<uint32_t>(ws.o_cnt));
  HIP_TRY(ctx, hipGetLastError());
  return ORCGPU_OK;
}

// The stable LSD radix sort of the row list, which starts in `a` and ends in ws.o_rows
int top_k_sort(const FilterCall& f, const FilterWorkspace& ws, const orcgpu_host::TopKWorkspace& tw, const orcgpu_host::TopKPlan& plan, uint32_t* a, uint32_t* b, uint64_t n_src) {
  orcgpu_ctx* ctx = f.ctx;
  hipStream_t st = ctx->stream;
  const FilterCol* d_cols = f.at<const FilterCol>(ws.o_cols);
  const unsigned long long* d_total = f.at<const unsigned long long>(ws.o_counters);
  uint32_t* d_hist = f.at<uint32_t>(tw.o_sort_hist);
  for (const orcgpu_host::TopKPass& p : orcgpu_host::top_k_sort_passes(plan.keys)) {
    const TopKKey key = plan.keys.key[p.key];
    hipLaunchKernelGGL(top_k_sort_hist_kernel, dim3(tw.sort_blocks), dim3(256), 0, st, key, p.byte, d_cols, f.B, f.W, n_src, (const uint32_t*)a, d_total, tw.cap, d_hist);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(group_wide_scan_kernel, dim3(1), dim3(1024), 0, st, d_hist, tw.sort_blocks * 256u, (uint32_t*)nullptr, 0u, (uint32_t*)nullptr);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(top_k_sort_scatter_kernel, dim3(tw.sort_blocks), dim3(256), 0, st, key, p.byte, d_cols, f.B, f.W, n_src, (const uint32_t*)a, b, d_total, tw.cap,
                       (const uint32_t*)d_hist);
    HIP_TRY(ctx, hipGetLastError());
    std::swap(a, b);
  }
  return a == f.at<uint32_t>(ws.o_rows) ? ORCGPU_OK : ORCGPU_UNEXPECTED;
}

// Open, evaluate, select, sort, the one wait, gather, adopt.  fplan: the row filter (null: none).  records (may be null): the key
// records of the rows handed out, in their order, top_k_stride(plan.keys.len) bytes apart.
int result_top_k_plan(orcgpu_ctx* ctx, orcgpu_result* r, const orcgpu_host::FilterPlan* fplan, const orcgpu_host::TopKPlan& plan, uint64_t* rows_seen, uint64_t* rows_kept,
                      uint64_t* rows_out, std::vector<uint8_t>* records, const char* const* column_names = nullptr, uint32_t n_names = 0) {
  static const orcgpu_host::FilterPlan no_filter;
  if (rows_seen) *rows_seen = 0;
  if (rows_kept) *rows_kept = 0;
  if (rows_out) *rows_out = 0;
  if (records) records->clear();
  if (r->status) return r->status;  // a failed decode is left as it is
  if (const int rc = filter_refuse(ctx, r)) return rc;
  FilterCall f{ctx, r, fplan ? *fplan : no_filter, column_names, n_names, fplan != nullptr};
  if (const int rc = filter_open(f, rows_seen)) return rc;
  const uint64_t cap = std::min<uint64_t>(plan.k, f.n_in);
  const FilterWorkspace ws = filter_workspace(f, cap);
  const orcgpu_host::TopKWorkspace tw(ws.bytes, plan.keys.len, plan.k, f.n_in);
  if (const int rc = filter_reserve(f, ws, tw.bytes, "the top-k selection")) return rc;
  if (!top_k_plan_in_bounds(plan, f)) {
    set_err(ctx, "top-k: a sort key's column is not decoded to the type the key was planned for");
    return ORCGPU_MISMATCHED_SCHEMA;
  }
  if (f.n_in >= 0xffffffffull) {
    set_err(ctx, "top-k: %llu input rows in one result", (unsigned long long)f.n_in);
    return ORCGPU_UNSUPPORTED;
  }
  std::vector<uint64_t> back(ws.n_counters, 0);
  TopKState state{};
  std::vector<uint8_t> recs(tw.recs_bytes);
  if (f.n_in) {
    hipStream_t st = ctx->stream;
    if (const int rc = filter_upload(f, ws)) return rc;
    if (f.has_filter)
      if (const int rc = filter_run_eval(f, ws)) return rc;
    const KeptRows rows = filter_kept_rows(f, ws);
    if (const int rc = top_k_select(f, ws, tw, plan, rows)) return rc;
    const uint32_t n_segs = (uint32_t)f.segs.size(), nb_max = (uint32_t)ws.nb_max;
    const FilterCol* d_cols = f.at<const FilterCol>(ws.o_cols);
    unsigned long long* d_counters = f.at<unsigned long long>(ws.o_counters);
    uint32_t *d_rows = f.at<uint32_t>(ws.o_rows), *d_rows2 = f.at<uint32_t>(tw.o_rows2);
    uint32_t* const d_first_list = plan.keys.len % 2 ? d_rows2 : d_rows;  // (an odd count of sort passes ends in the other list)
    if (const int rc = enc_scan(ctx, st, f.at<const uint32_t>(ws.o_cnt), ws.n_words, f.at<uint64_t>(ws.o_sums), reinterpret_cast<uint64_t*>(d_counters), f.at<uint64_t>(ws.o_woff)))
      return rc;
    hipLaunchKernelGGL(filter_place_kernel, dim3((uint32_t)((f.n_in + 255) / 256)), dim3(256), 0, st, f.at<const unsigned long long>(tw.o_final),
                       f.at<const unsigned long long>(ws.o_woff), f.at<const SelBatch>(ws.o_segs), f.at<const unsigned long long>(ws.o_first), n_segs, f.n_in, d_first_list);
    HIP_TRY(ctx, hipGetLastError());
    const uint64_t n_src = top_k_source_rows(f);
    if (const int rc = top_k_sort(f, ws, tw, plan, d_first_list, d_first_list == d_rows ? d_rows2 : d_rows, n_src)) return rc;
    hipLaunchKernelGGL(top_k_records_kernel, dim3((tw.cap + 255) / 256), dim3(256), 0, st, plan.keys, d_cols, f.B, f.W, n_src, (const uint32_t*)d_rows,
                       (const unsigned long long*)d_counters, tw.cap, tw.stride, f.at<uint8_t>(tw.o_recs));
    HIP_TRY(ctx, hipGetLastError());
    for (uint32_t o = 0; o < f.nc; o += 65535u)
      hipLaunchKernelGGL(filter_count_kernel, dim3(nb_max, std::min<uint32_t>(65535u, f.nc - o)), dim3(256), 0, st, d_cols + o, (const uint32_t*)d_rows,
                         (const unsigned long long*)d_counters, f.B, f.W, nb_max, d_counters + 1 + (uint64_t)o * nb_max, d_counters + 1 + ((uint64_t)f.nc + o) * nb_max);
    HIP_TRY(ctx, hipGetLastError());
    // ---- the one wait: the winners' count with the null counts and string bytes per output batch, the select's state (the rows
    // the predicate kept), and the key records of at most min(k, n_in) rows ----
    HIP_TRY(ctx, hipMemcpyAsync(back.data(), d_counters, ws.n_counters * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(&state, f.at<TopKState>(tw.o_state), sizeof(state), hipMemcpyDeviceToHost, st));
    if (tw.recs_bytes) HIP_TRY(ctx, hipMemcpyAsync(recs.data(), f.at<uint8_t>(tw.o_recs), tw.recs_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  const uint64_t out_rows = back[0], kept = state.kept;
  if (kept > f.n_in || out_rows != std::min<uint64_t>(plan.k, kept)) {
    set_err(ctx, "top-k: %llu rows selected of %llu kept of %llu", (unsigned long long)out_rows, (unsigned long long)kept, (unsigned long long)f.n_in);
    return ORCGPU_UNEXPECTED;
  }
  FilterOutput out = filter_place_output(f.descs.data(), back.data(), f.nc, ws.nb_max, out_rows, f.B, f.W);
  r->filt_used = out_rows ? out.arena_bytes : 0;
  if (out_rows)
    if (const int rc = filter_run_gather(f, ws, out, out_rows)) return rc;
  filter_adopt_output(r, out, out_rows);
  if (rows_kept) *rows_kept = kept;
  if (rows_out) *rows_out = out_rows;
  if (records) {
    recs.resize(out_rows * tw.stride);
    records->swap(recs);
  }
  return ORCGPU_OK;
}

// The plan of a key list against a decoded result's columns
int result_compile_top_k(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_sort_key* keys, uint32_t n_keys, uint32_t k, const char* const* column_names,
                         orcgpu_host::TopKPlan& plan) {
  const std::vector<orcgpu_host::AggCol> cols = result_agg_cols(r);
  const int rc = orcgpu_host::top_k_compile(keys, n_keys, k, column_names, cols.data(), (uint32_t)cols.size(), plan);
  if (rc) set_err(ctx, "%s", plan.err);
  return rc;
}

}  // namespace

extern "C" int orcgpu_result_top_k(orcgpu_ctx* ctx, orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes, const char* const* column_names,
                                   uint32_t n_columns, const orcgpu_sort_key* keys, uint32_t n_keys, uint32_t k, uint64_t* rows_kept, uint64_t* rows_out) {
  if (!ctx || !r || (n_nodes && !nodes) || (n_columns && !column_names)) return ORCGPU_INVALID_ARGUMENT;
  if (rows_kept) *rows_kept = 0;
  if (rows_out) *rows_out = 0;
  if (r->status) return r->status;
  if (n_columns != r->cols.size()) {
    set_err(ctx, "top-k: %u column names for a result of %zu columns", n_columns, r->cols.size());
    return ORCGPU_INVALID_ARGUMENT;
  }
  orcgpu_host::TopKPlan plan;
  if (const int rc = result_compile_top_k(ctx, r, keys, n_keys, k, column_names, plan)) return rc;
  orcgpu_host::FilterPlan fplan;
  if (n_nodes)
    if (const int rc = result_compile_filter(ctx, r, nodes, n_nodes, column_names, fplan)) return rc;
  return result_top_k_plan(ctx, r, n_nodes ? &fplan : nullptr, plan, nullptr, rows_kept, rows_out, nullptr, column_names, n_columns);
}
