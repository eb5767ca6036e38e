// orcgpu_filter.inc -- the row filter at the seam: orcgpu_result_filter and what the file reader calls per stripe.  The plan
// compiler is orcgpu_filter_plan.inc (host only), the kernels device/filter_kernels.hip.
//
// One filtered result costs ONE host wait: behind evaluate -> scan -> place -> count the host fetches the kept row count with
// the per-batch null counts and string byte totals (result_filter_plan, "the filter's one wait"); with them it lays the
// output arena out compactly -- so that a copy back moves the kept rows' bytes and no more -- and enqueues the gather, which
// nobody waits for: orcgpu_result_fetch_async orders its copies behind the decode stream.
#include "orcgpu_filter_plan.inc"
namespace {

int enc_scan(orcgpu_ctx* ctx, hipStream_t st, const uint32_t* d_in, uint64_t count, uint64_t* d_sums, uint64_t* d_total, uint64_t* d_out);

int result_filter_plan(orcgpu_ctx* ctx, orcgpu_result* r, const orcgpu_host::FilterPlan& plan, uint64_t* rows_seen, uint64_t* rows_kept,
                       const char* const* column_names = nullptr, uint32_t n_names = 0) {
  if (rows_seen) *rows_seen = 0;
  if (rows_kept) *rows_kept = 0;
  if (r->status) return r->status;  // a failed decode is left as it is
  if (r->hold && orcgpu_hold::hold_exported(r->hold)) {
    set_err(ctx, "a result that exported device batches still view cannot be filtered");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (r->filtered) {
    set_err(ctx, "a row filter has already been applied to this result");
    return ORCGPU_INVALID_ARGUMENT;
  }
  const uint32_t nc = (uint32_t)r->cols.size();
  for (uint32_t c = 0; c < nc; c++) {
    const ColumnOut& co = r->cols[c];
    if (co.is_struct || co.is_union || co.is_list || co.elem || co.parent >= 0 || !r->subs.empty()) {
      set_err(ctx, "row filter: column %u of the result is nested (Struct / List / Map / Union are not filtered)", co.column_id);
      return ORCGPU_UNSUPPORTED;
    }
    if (!co.is_bool && !co.is_string && co.width != 1 && co.width != 2 && co.width != 4 && co.width != 8 && co.width != 16) {
      set_err(ctx, "row filter: column %u has values of %u bytes", co.column_id, co.width);
      return ORCGPU_UNSUPPORTED;
    }
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t B = r->batch, W = r->words_per_batch;
  // ---- the input rows: the stripe's, or those of a row selection's batches ----
  std::vector<SelBatch> segs;
  std::vector<uint64_t> seg_first;
  uint64_t n_in = r->n_rows;
  if (r->selected) {
    n_in = 0;
    for (auto& b : r->sel) {
      seg_first.push_back(n_in);
      segs.push_back(b);
      n_in += b.len;
    }
  }
  const uint32_t n_segs = (uint32_t)segs.size();
  const uint64_t n_words = (n_in + 63) / 64, nb_max = (n_in + B - 1) / B;
  if (rows_seen) *rows_seen = n_in;
  // ---- temporaries: tables that go up in one copy, then what the kernels leave ----
  Bump t;
  const uint64_t o_prog = t.take(plan.prog.size() * sizeof(FilterInsn) + 16), o_lits = t.take(plan.lits.size() + 16);
  const uint64_t o_cols = t.take((uint64_t)nc * sizeof(FilterCol) + 16), o_segs = t.take((uint64_t)n_segs * sizeof(SelBatch) + 16);
  const uint64_t o_first = t.take((uint64_t)n_segs * 8 + 16);
  std::vector<uint64_t> o_cbase(nc, 0);
  const uint32_t src_batches = r->selected ? r->full_batches : r->n_batches;  // uniform batches of the decode
  for (uint32_t c = 0; c < nc; c++)
    if (r->cols[c].is_string) o_cbase[c] = t.take((uint64_t)src_batches * 8 + 16);
  const uint64_t up_bytes = t.off;
  const uint64_t o_keep = t.take(n_words * 8 + 16), o_cnt = t.take(n_words * 4 + 16), o_woff = t.take(n_words * 8 + 16);
  const uint64_t o_sums = t.take(((n_words + 2047) / 2048) * 8 + 16);
  const uint64_t n_counters = 1 + 2ull * nc * nb_max;  // the kept row count, then null counts and string bytes [column][batch]
  const uint64_t o_counters = t.take(n_counters * 8 + 16), o_rows = t.take(n_in * 4 + 16);
  // (the LIKE and IN leaves' planes of match bits, numbered together and laid out like `keep`: part of this workspace, which
  // only ever grows)
  uint32_t n_like = 0, n_set = 0;
  for (auto& in : plan.prog) {
    n_like += in.op == FOP_LIKE && in.cmp != LIKE_ALL;
    n_set += in.op == FOP_IN && !(in.cmp & IN_NO_TABLE);
  }
  const uint32_t n_planes = n_like + n_set;
  const uint64_t o_like = t.take((uint64_t)n_planes * n_words * 8 + 16);
  // (the second upload, behind the wait: the gather's jobs and the char bases of the output batches)
  const uint64_t o_jobs = t.take((uint64_t)nc * sizeof(FilterGatherJob) + 16), o_obase = t.take((uint64_t)nc * nb_max * 8 + 16);
  if (!r->filt_tmp.ensure(t.off + kAlign)) {
    set_err(ctx, "hipMalloc(%llu) for the row filter failed", (unsigned long long)t.off);
    return ORCGPU_HIP_ERROR;
  }
  uint8_t* X = r->filt_tmp.p;
  std::vector<uint8_t> host(up_bytes, 0);
  if (!plan.prog.empty()) memcpy(host.data() + o_prog, plan.prog.data(), plan.prog.size() * sizeof(FilterInsn));
  if (!plan.lits.empty()) memcpy(host.data() + o_lits, plan.lits.data(), plan.lits.size());
  if (n_segs) {
    memcpy(host.data() + o_segs, segs.data(), (size_t)n_segs * sizeof(SelBatch));
    memcpy(host.data() + o_first, seg_first.data(), (size_t)n_segs * 8);
  }
  std::vector<FilterCol> fcols(nc);
  for (uint32_t c = 0; c < nc; c++) {
    const ColumnOut& co = r->cols[c];
    const uint8_t* A = r->arena[co.lane].p;
    FilterCol& f = fcols[c];
    memset(&f, 0, sizeof(f));
    f.validity = co.has_present && r->n_rows ? reinterpret_cast<const unsigned long long*>(A + co.validity_off) : nullptr;
    f.width = co.width;
    if (co.is_bool) {
      f.kind = FKIND_BOOL;
      f.values = A + co.values_off;
    } else if (co.is_string) {
      f.kind = FKIND_STRING;
      f.offsets = reinterpret_cast<const int32_t*>(A + co.offsets_off);
      f.chars = (co.values_in_chars ? r->chars[co.lane].p : A) + co.values_off;
      f.char_base = reinterpret_cast<const unsigned long long*>(X + o_cbase[c]);
      for (size_t k = 0; k < co.char_base.size() && k < src_batches; k++) reinterpret_cast<uint64_t*>(host.data() + o_cbase[c])[k] = co.char_base[k];
    } else {
      const int ot = co.orc_type;
      const bool is_int = ot == ORCGPU_T_BYTE || ot == ORCGPU_T_SHORT || ot == ORCGPU_T_INT || ot == ORCGPU_T_LONG || ot == ORCGPU_T_DATE;
      const bool is_float = ot == ORCGPU_T_FLOAT || ot == ORCGPU_T_DOUBLE;
      // (a value narrower or wider than the type's own -- with_schema -- is still compared as what it is: 1 / 2 / 4 / 8 bytes)
      // (a Timestamp decoded to an int64 unit is compared as the integer it is; decoded to Decimal128(38, 9) it is not compared)
      const bool is_ts = (ot == ORCGPU_T_TIMESTAMP || ot == ORCGPU_T_TIMESTAMP_INSTANT) && co.ts_unit <= 3 && co.width == 8;
      const bool is_dec = ot == ORCGPU_T_DECIMAL && co.width == 16;
      f.kind = (is_int && co.width <= 8) || is_ts ? FKIND_INT
               : (is_float && (co.width == 4 || co.width == 8) ? FKIND_FLOAT : (is_dec ? FKIND_DEC128 : FKIND_OTHER));
      f.values = A + co.values_off;
    }
  }
  for (auto& in : plan.prog) {  // (the plan was compiled against these columns' types; what the decode made of them must fit)
    if (!fop_reads_values(in.op)) continue;
    if (in.col < nc && r->cols[in.col].dict_out) {  // (string predicates evaluated on the entries: not yet)
      if (column_names && in.col < n_names) set_err(ctx, "row filter: column '%s' is read as a dictionary column: a comparison on its keys is not supported", column_names[in.col]);
      else set_err(ctx, "row filter: column %u is read as a dictionary column: a comparison on its keys is not supported", r->cols[in.col].column_id);
      return ORCGPU_UNSUPPORTED;
    }
    const uint32_t want = in.op == FOP_IN ? (uint32_t)in.lo : in.op == FOP_CMP_INT ? FKIND_INT : in.op == FOP_CMP_FLOAT ? FKIND_FLOAT : in.op == FOP_CMP_BOOL ? FKIND_BOOL : in.op == FOP_CMP_DEC128 ? FKIND_DEC128 : FKIND_STRING;
    if (in.col >= nc || fcols[in.col].kind != want) {
      set_err(ctx, "row filter: column %u is not decoded to the type its comparison needs", in.col < nc ? r->cols[in.col].column_id : in.col);
      return ORCGPU_MISMATCHED_SCHEMA;
    }
  }
  if (nc) memcpy(host.data() + o_cols, fcols.data(), (size_t)nc * sizeof(FilterCol));
  const FilterCol* d_cols = reinterpret_cast<const FilterCol*>(X + o_cols);
  const SelBatch* d_segs = reinterpret_cast<const SelBatch*>(X + o_segs);
  const unsigned long long* d_first = reinterpret_cast<const unsigned long long*>(X + o_first);
  unsigned long long* d_counters = reinterpret_cast<unsigned long long*>(X + o_counters);
  uint32_t* d_rows = reinterpret_cast<uint32_t*>(X + o_rows);
  std::vector<uint64_t> back(n_counters, 0);
  if (n_in) {
    HIP_TRY(ctx, ctx->upload(X, host.data(), up_bytes, st));
    HIP_TRY(ctx, hipMemsetAsync(d_counters, 0, n_counters * 8, st));
    const uint32_t eval_blocks = (uint32_t)std::min<uint64_t>((n_words + 3) / 4, 16384);
    if (n_like) {  // the matcher first: the evaluation reads its bits
      hipLaunchKernelGGL(filter_like_kernel, dim3(eval_blocks, n_planes), dim3(256), 0, st, reinterpret_cast<const FilterInsn*>(X + o_prog), (uint32_t)plan.prog.size(),
                         reinterpret_cast<const uint8_t*>(X + o_lits), d_cols, d_segs, d_first, n_segs, n_in, B, W, reinterpret_cast<unsigned long long*>(X + o_like));
      HIP_TRY(ctx, hipGetLastError());
    }
    if (n_set) {  // ... and the set membership of the IN leaves (a block of either kernel whose plane is the other's leaves at once)
      hipLaunchKernelGGL(filter_in_kernel, dim3(eval_blocks, n_planes), dim3(256), 0, st, reinterpret_cast<const FilterInsn*>(X + o_prog), (uint32_t)plan.prog.size(),
                         reinterpret_cast<const uint8_t*>(X + o_lits), d_cols, d_segs, d_first, n_segs, n_in, B, W, reinterpret_cast<unsigned long long*>(X + o_like));
      HIP_TRY(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(filter_eval_kernel, dim3(eval_blocks), dim3(256), 0, st, reinterpret_cast<const FilterInsn*>(X + o_prog), (uint32_t)plan.prog.size(),
                       reinterpret_cast<const uint8_t*>(X + o_lits), d_cols, d_segs, d_first, n_segs, n_in, B, W,
                       reinterpret_cast<unsigned long long*>(X + o_keep), reinterpret_cast<uint32_t*>(X + o_cnt),
                       reinterpret_cast<const unsigned long long*>(X + o_like));
    HIP_TRY(ctx, hipGetLastError());
    int rc = enc_scan(ctx, st, reinterpret_cast<const uint32_t*>(X + o_cnt), n_words, reinterpret_cast<uint64_t*>(X + o_sums),
                      reinterpret_cast<uint64_t*>(d_counters), reinterpret_cast<uint64_t*>(X + o_woff));
    if (rc) return rc;
    hipLaunchKernelGGL(filter_place_kernel, dim3((uint32_t)((n_in + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const unsigned long long*>(X + o_keep),
                       reinterpret_cast<const unsigned long long*>(X + o_woff), d_segs, d_first, n_segs, n_in, d_rows);
    HIP_TRY(ctx, hipGetLastError());
    for (uint32_t o = 0; o < nc; o += 65535u)
      hipLaunchKernelGGL(filter_count_kernel, dim3((uint32_t)nb_max, std::min<uint32_t>(65535u, nc - o)), dim3(256), 0, st, d_cols + o, d_rows,
                         reinterpret_cast<const unsigned long long*>(d_counters), B, W, (uint32_t)nb_max, d_counters + 1 + (uint64_t)o * nb_max,
                         d_counters + 1 + ((uint64_t)nc + o) * nb_max);
    HIP_TRY(ctx, hipGetLastError());
    // ---- the filter's one wait: the kept row count, null counts and string bytes per output batch ----
    HIP_TRY(ctx, hipMemcpyAsync(back.data(), d_counters, n_counters * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  const uint64_t kept = back[0];
  if (kept > n_in) {
    set_err(ctx, "row filter: %llu rows kept of %llu", (unsigned long long)kept, (unsigned long long)n_in);
    return ORCGPU_UNEXPECTED;
  }
  const uint32_t nbo = (uint32_t)((kept + B - 1) / B);
  auto nulls_of = [&](uint32_t c, uint32_t k) { return back[1 + (uint64_t)c * nb_max + k]; };
  auto bytes_of = [&](uint32_t c, uint32_t k) { return back[1 + ((uint64_t)nc + c) * nb_max + k]; };
  // ---- the output arena, compact: per column what a decode of `kept` rows would hold ----
  Bump a;
  std::vector<FilterGatherJob> jobs(nc);
  std::vector<uint64_t> obase((size_t)nc * nb_max, 0);
  struct Place {
    uint64_t validity = 0, values = 0, offsets = 0, dict_offsets = 0, dict_values = 0;
    bool has_validity = false;
  };
  std::vector<Place> place(nc);
  int status = 0;
  uint32_t err_batch = 0, err_col = 0;
  for (uint32_t c = 0; c < nc; c++) {
    const ColumnOut& co = r->cols[c];
    Place& p = place[c];
    uint64_t nulls = 0, bytes = 0;
    for (uint32_t k = 0; k < nbo; k++) {
      nulls += nulls_of(c, k);
      obase[(size_t)c * nb_max + k] = bytes;
      bytes += bytes_of(c, k);
      // OffsetOverflow (string.rs:139-140: the offsets of a batch are i32), as the decoder's check of its uniform batches
      if (co.is_string && bytes_of(c, k) > 0x7fffffffull && (!status || k < err_batch)) {
        status = ORCGPU_OFFSET_OVERFLOW;
        err_batch = k;
        err_col = c;
      }
    }
    p.has_validity = nulls != 0;
    if (p.has_validity) p.validity = a.take((uint64_t)nbo * W * 8 + 16);
    if (co.is_bool) p.values = a.take((uint64_t)nbo * W * 8 + 16);
    else if (co.is_string) {
      p.offsets = a.take((uint64_t)nbo * (B + 1) * 4 + 16);
      p.values = a.take(bytes + 16);
    } else p.values = a.take(kept * co.width + 16);
    if (co.dict_out && co.dict_decoded) {  // the stripe's dictionary goes along untouched: this arena is all that is copied back
      p.dict_offsets = a.take((co.dict_len + 1) * 4 + 16);
      p.dict_values = a.take(co.dict_bytes + 16);
    }
  }
  r->filt_used = kept ? a.off : 0;
  if (kept) {
    if (!r->filt_arena.ensure(a.off + kAlign)) {
      set_err(ctx, "hipMalloc(%llu) for the filtered rows failed", (unsigned long long)a.off);
      return ORCGPU_HIP_ERROR;
    }
    uint8_t* O = r->filt_arena.p;
    for (uint32_t c = 0; c < nc; c++) {
      FilterGatherJob& j = jobs[c];
      memset(&j, 0, sizeof(j));
      j.src = fcols[c];
      const Place& p = place[c];
      j.out_validity = p.has_validity ? reinterpret_cast<unsigned long long*>(O + p.validity) : nullptr;
      j.out_values = O + p.values;
      j.out_chars = O + p.values;
      j.out_offsets = reinterpret_cast<int32_t*>(O + p.offsets);
      j.out_char_base = reinterpret_cast<const unsigned long long*>(X + o_obase) + (uint64_t)c * nb_max;
    }
    for (uint32_t c = 0; c < nc; c++) {
      const ColumnOut& co = r->cols[c];
      if (!co.dict_out || !co.dict_decoded) continue;
      const uint8_t* A = r->arena[co.lane].p;
      HIP_TRY(ctx, hipMemcpyAsync(O + place[c].dict_offsets, A + co.dict_offsets_off, (co.dict_len + 1) * 4, hipMemcpyDeviceToDevice, st));
      if (co.dict_bytes) HIP_TRY(ctx, hipMemcpyAsync(O + place[c].dict_values, A + co.dict_values_off, co.dict_bytes, hipMemcpyDeviceToDevice, st));
    }
    std::vector<uint8_t> up2(o_obase + obase.size() * 8 - o_jobs, 0);
    memcpy(up2.data(), jobs.data(), (size_t)nc * sizeof(FilterGatherJob));
    memcpy(up2.data() + (o_obase - o_jobs), obase.data(), obase.size() * 8);
    HIP_TRY(ctx, ctx->upload(X + o_jobs, up2.data(), up2.size(), st));
    for (uint32_t o = 0; o < nc; o += 65535u)
      hipLaunchKernelGGL(filter_gather_kernel, dim3(nbo, std::min<uint32_t>(65535u, nc - o)), dim3(256), 0, st,
                         reinterpret_cast<const FilterGatherJob*>(X + o_jobs) + o, d_rows, kept, B, W);
    HIP_TRY(ctx, hipGetLastError());
  }
  // ---- the result now speaks in the kept rows: uniform batches in the filter's own arena ----
  r->arrow_bytes = 0;
  for (uint32_t c = 0; c < nc; c++) {
    ColumnOut& co = r->cols[c];
    const Place& p = place[c];
    co.lane = 0;
    co.values_in_chars = false;
    co.validity_off = p.validity;
    co.values_off = p.values;
    co.offsets_off = p.offsets;
    if (co.dict_out) {
      if (!kept) {  // (no batch is left to refer to it)
        co.dict_len = co.dict_bytes = 0;
        co.dict_decoded = false;
      }
      co.dict_offsets_off = kept ? p.dict_offsets : 0;
      co.dict_values_off = kept ? p.dict_values : 0;
      if (co.dict_decoded) r->arrow_bytes += (co.dict_len + 1) * 4 + co.dict_bytes;
    }
    co.null_counts.assign(nbo, 0);
    co.char_base.assign(co.is_string ? nbo : 0, 0);
    co.char_total.assign(co.is_string ? nbo : 0, 0);
    co.sel_nulls.clear();
    co.sel_char_start.clear();
    co.sel_char_total.clear();
    for (uint32_t k = 0; k < nbo; k++) {
      const uint64_t rows = std::min<uint64_t>(B, kept - (uint64_t)k * B);
      co.null_counts[k] = nulls_of(c, k);
      if (co.is_string) {
        co.char_base[k] = obase[(size_t)c * nb_max + k];
        co.char_total[k] = bytes_of(c, k);
      }
      r->arrow_bytes += co.is_string ? co.char_total[k] + 4 * (rows + 1) : (co.is_bool ? (rows + 7) / 8 : rows * co.width);
      if (co.null_counts[k]) r->arrow_bytes += (rows + 7) / 8;
    }
  }
  r->n_rows = kept;
  r->n_batches = nbo;
  r->selected = false;
  r->sel.clear();
  r->filtered = true;
  r->mirror_valid = false;
  r->dev_ready_recorded = false;
  if (status) {
    r->status = status;
    r->err_batch = err_batch;
    r->err_col = err_col;
  }
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
  std::vector<int32_t> kinds(n_columns), params(n_columns, 0);
  for (uint32_t c = 0; c < n_columns; c++) {
    const ColumnOut& co = r->cols[c];
    kinds[c] = co.orc_type;
    params[c] = co.orc_type == ORCGPU_T_DECIMAL ? (int32_t)co.scale : co.ts_unit;  // what Decimal128 / TimestampNs literals are brought to
  }
  orcgpu_host::FilterPlan plan;
  int rc = orcgpu_host::filter_compile(nodes, n_nodes, column_names, kinds.data(), n_columns, plan, params.data());
  if (rc) {
    set_err(ctx, "%s", plan.err);
    return rc;
  }
  return result_filter_plan(ctx, r, plan, nullptr, rows_kept, column_names, n_columns);
}
