// orcgpu_select.inc -- RowSelection at the seam: the stepping of NaiveStripeDecoder::next_with_row_selection
// (array_decoder/mod.rs:302-365), RowSelection's normalisation and split_off (row_selection.rs:278-314, :466-482).
#include "orcgpu_selection.inc"
namespace {

int result_select_batches(orcgpu_ctx* ctx, orcgpu_result* r, std::vector<SelBatch> batches);
int result_select(orcgpu_ctx* ctx, orcgpu_result* r, const std::vector<RowSel>& sel) {
  return result_select_batches(ctx, r, sel_batches(sel, r->n_rows, r->batch));
}
// ... with the batches given as row ranges of the result (each at most `batch` rows, inside the result's rows)
int result_select_batches(orcgpu_ctx* ctx, orcgpu_result* r, std::vector<SelBatch> batches) {
  if (r->hold && orcgpu_hold::hold_exported(r->hold)) {
    set_err(ctx, "a result that exported device batches still view cannot be selected on");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (r->selected) {
    set_err(ctx, "a row selection has already been applied to this result");
    return ORCGPU_INVALID_ARGUMENT;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  for (auto& b : batches)
    if (b.start > r->n_rows || b.len > r->n_rows - b.start || b.len > r->batch) return ORCGPU_INVALID_ARGUMENT;
  const uint32_t nb = (uint32_t)batches.size(), nc = (uint32_t)r->cols.size();
  const uint32_t B = r->batch, W = r->words_per_batch;
  // ---- layout of the per-batch buffers ----
  Bump b;
  const uint64_t o_batches = b.take((uint64_t)nb * sizeof(SelBatch) + 16), o_jobs = b.take((uint64_t)nc * sizeof(SelJob) + 16);
  std::vector<uint64_t> o_nulls(nc, 0), o_cstart(nc, 0), o_ctotal(nc, 0), o_cbase(nc, 0);
  // (the counters that come back to the host -- null counts, first byte and byte total of every column's batches -- lie together:
  // one copy)
  const uint64_t o_counters = b.take((uint64_t)nc * 3 * nb * 8 + 16);
  for (uint32_t c = 0; c < nc; c++) {
    ColumnOut& co = r->cols[c];
    co.sel_validity_off = co.has_present ? b.take((uint64_t)nb * W * 8 + 16) : 0;
    co.sel_bool_off = co.is_bool ? b.take((uint64_t)nb * W * 8 + 16) : 0;
    // (a List / Map is stepped like a string column, list.rs:89 / map.rs:106: its offsets count ELEMENTS; a selected batch's
    // elements are a range of the stripe's element arrays, which the exported List / Map array points into)
    co.sel_offsets_off = (co.is_string || co.is_list) ? b.take((uint64_t)nb * (B + 1) * 4 + 16) : 0;
    o_nulls[c] = o_counters + ((uint64_t)c * 3 + 0) * nb * 8;
    o_cstart[c] = o_counters + ((uint64_t)c * 3 + 1) * nb * 8;
    o_ctotal[c] = o_counters + ((uint64_t)c * 3 + 2) * nb * 8;
    o_cbase[c] = b.take((uint64_t)r->n_batches * 8 + 16);
  }
  r->sel_used = b.off;
  if (!r->sel_arena.ensure(b.off + kAlign)) {
    set_err(ctx, "hipMalloc(%llu) for the row selection failed", (unsigned long long)b.off);
    return ORCGPU_HIP_ERROR;
  }
  uint8_t* X = r->sel_arena.p;
  hipStream_t st = ctx->stream;
  std::vector<SelJob> jobs(nc);
  std::vector<uint8_t> host(b.off, 0);  // what goes up in one copy: batch table, jobs, char bases, zeroed counters
  memcpy(host.data() + o_batches, batches.data(), (size_t)nb * sizeof(SelBatch));
  for (uint32_t c = 0; c < nc; c++) {
    ColumnOut& co = r->cols[c];
    const uint8_t* A = r->arena[co.lane].p;
    SelJob& j = jobs[c];
    memset(&j, 0, sizeof(j));
    j.src_validity = co.has_present && r->n_rows ? reinterpret_cast<const unsigned long long*>(A + co.validity_off) : nullptr;
    j.src_bool = co.is_bool ? reinterpret_cast<const unsigned long long*>(A + co.values_off) : nullptr;
    j.src_offsets = (co.is_string || co.is_list) ? reinterpret_cast<const int32_t*>(A + co.offsets_off) : nullptr;
    j.src_char_base = reinterpret_cast<const unsigned long long*>(X + o_cbase[c]);
    j.out_validity = reinterpret_cast<unsigned long long*>(X + co.sel_validity_off);
    j.out_bool = reinterpret_cast<unsigned long long*>(X + co.sel_bool_off);
    j.out_offsets = reinterpret_cast<int32_t*>(X + co.sel_offsets_off);
    j.out_nulls = reinterpret_cast<unsigned long long*>(X + o_nulls[c]);
    j.out_char_start = reinterpret_cast<unsigned long long*>(X + o_cstart[c]);
    j.out_char_total = reinterpret_cast<unsigned long long*>(X + o_ctotal[c]);
    j.batch = B;
    j.words_per_batch = W;
    if (co.is_string || co.is_list)
      for (uint32_t k = 0; k < r->n_batches && k < co.char_base.size(); k++) reinterpret_cast<uint64_t*>(host.data() + o_cbase[c])[k] = co.char_base[k];
  }
  memcpy(host.data() + o_jobs, jobs.data(), (size_t)nc * sizeof(SelJob));
  HIP_TRY(ctx, ctx->upload(X, host.data(), b.off, st));
  if (nb && nc) {
    for (uint32_t o = 0; o < nc; o += 65535u)
      hipLaunchKernelGGL(select_build_kernel, dim3(nb, std::min<uint32_t>(65535u, nc - o)), dim3(256), 0, st,
                         reinterpret_cast<const SelJob*>(X + o_jobs) + o, reinterpret_cast<const SelBatch*>(X + o_batches));
    HIP_TRY(ctx, hipGetLastError());
  }
  std::vector<uint64_t> back((size_t)nc * 3 * nb + 1);
  if (nb && nc) HIP_TRY(ctx, hipMemcpyAsync(back.data(), X + o_counters, (size_t)nc * 3 * nb * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  // ---- the result now speaks in selected batches ----
  r->full_batches = r->n_batches;
  r->full_status = r->status;
  r->full_err_batch = r->err_batch;
  r->full_err_col = r->err_col;
  r->arrow_bytes = 0;
  for (uint32_t c = 0; c < nc; c++) {
    ColumnOut& co = r->cols[c];
    co.sel_nulls.assign(back.begin() + ((size_t)c * 3 + 0) * nb, back.begin() + ((size_t)c * 3 + 1) * nb);
    co.sel_char_start.assign(back.begin() + ((size_t)c * 3 + 1) * nb, back.begin() + ((size_t)c * 3 + 2) * nb);
    co.sel_char_total.assign(back.begin() + ((size_t)c * 3 + 2) * nb, back.begin() + ((size_t)c * 3 + 3) * nb);
    for (uint32_t k = 0; k < nb; k++) {
      const uint64_t rows = batches[k].len;
      r->arrow_bytes += co.is_string ? co.sel_char_total[k] + 4 * (rows + 1) : (co.is_list ? 4 * (rows + 1) : (co.is_bool ? (rows + 7) / 8 : rows * co.width));
      if (co.sel_nulls[k]) r->arrow_bytes += (rows + 7) / 8;
    }
    if (co.dict_out && nb) r->arrow_bytes += (co.dict_len + 1) * 4 + co.dict_bytes;  // the stripe's dictionary, once
  }
  if (r->status) {
    // The stripe failed in uniform batch err_batch, i.e. at or behind row err_batch * batch_size: the selected batches that
    // end before that row are good; the first one that reaches it carries the error (a failure inside a skipped run
    // surfaces when the next batch is asked for, mod.rs:329-333).
    const uint64_t bad_row = (uint64_t)r->err_batch * B;
    uint32_t k = 0;
    while (k < nb && batches[k].start + batches[k].len <= bad_row) k++;
    r->err_batch = k;
  }
  r->sel = std::move(batches);
  r->n_batches = nb;
  r->selected = true;
  r->mirror_valid = false;
  r->dev_ready_recorded = false;
  return ORCGPU_OK;
}

}  // namespace

// Host only (no GPU needed): the batches a selection yields on a stripe, and what is left of the selection for the next
// stripe -- the stepping itself, exported so that it can be checked against a restatement of the reference's loop.
extern "C" int orcgpu_selection_batches(const orcgpu_row_selector* selectors, uint32_t n, uint64_t stripe_rows, uint32_t batch_size,
                                        uint64_t* starts, uint32_t* lens, uint32_t cap, uint32_t* n_out, orcgpu_row_selector* rest, uint32_t rest_cap,
                                        uint32_t* n_rest) {
  if ((n && !selectors) || !n_out) return ORCGPU_INVALID_ARGUMENT;
  std::vector<RowSel> all = sel_normalise(selectors, n);
  std::vector<RowSel> mine = sel_split_off(all, stripe_rows);
  std::vector<SelBatch> b = sel_batches(mine, stripe_rows, batch_size ? batch_size : 8192);
  *n_out = (uint32_t)b.size();
  for (uint32_t i = 0; i < b.size() && i < cap; i++) {
    if (starts) starts[i] = b[i].start;
    if (lens) lens[i] = b[i].len;
  }
  if (n_rest) *n_rest = (uint32_t)all.size();
  for (uint32_t i = 0; i < all.size() && i < rest_cap && rest; i++) {
    rest[i].row_count = all[i].row_count;
    rest[i].skip = all[i].skip ? 1 : 0;
  }
  return ORCGPU_OK;
}

extern "C" int orcgpu_result_select(orcgpu_ctx* ctx, orcgpu_result* r, const orcgpu_row_selector* selectors, uint32_t n) {
  if (!ctx || !r || (n && !selectors)) return ORCGPU_INVALID_ARGUMENT;
  return result_select(ctx, r, sel_normalise(selectors, n));
}

extern "C" int orcgpu_timezone_offsets(const char* name, const int64_t* instants, uint32_t n, int32_t* offsets, int64_t* orc_epoch) {
  if (!name || (n && (!instants || !offsets))) return ORCGPU_INVALID_ARGUMENT;
  TzTable T;
  if (!find_timezone(name, T)) return ORCGPU_UNSUPPORTED;
  for (uint32_t i = 0; i < n; i++) offsets[i] = T.offset_at(instants[i]);
  if (orc_epoch) *orc_epoch = tz_orc_epoch(T);
  return ORCGPU_OK;
}
