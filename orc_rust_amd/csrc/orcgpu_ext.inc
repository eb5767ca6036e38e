// orcgpu_ext.inc -- planner/launch hooks for strings, decimals and compressed streams.
namespace {

int version_class(const orcgpu_column& c) {
  // column.rs:52-59: DIRECT / DICTIONARY -> RLE v1, *_V2 -> RLE v2
  return (c.encoding == ORCGPU_ENC_DIRECT_V2 || c.encoding == ORCGPU_ENC_DICTIONARY_V2) ? JC_RLE2 : JC_RLE1;
}
uint8_t class_codec(int cls) { return cls == JC_RLE2 ? CODEC_RLE2 : (cls == JC_RLE1 ? CODEC_RLE1 : CODEC_BYTE); }

// ---- strings / binary / decimal planning --------------------------------------------------------------
bool is_dict_encoding(const orcgpu_column& c) { return c.encoding == ORCGPU_ENC_DICTIONARY || c.encoding == ORCGPU_ENC_DICTIONARY_V2; }

int plan_column_ext(Plan& P, ColPlan& cp, ColumnOut& co, orcgpu_staged* s, orcgpu_result* r, int vcls) {
  const orcgpu_column& c = cp.c;
  const uint64_t n = cp.n_rows;
  const int si = cp.stripe, ci = cp.col;
  Bump& RB = P.result_bump[si];
  const int t = c.orc_type;
  if (is_string_type(t)) {
    const bool dout = cp.dict_out;
    // (dictionary output: the result holds one int32 key per row where the Utf8 path holds per-batch offsets)
    if (dout) {
      co.dict_decoded = true;
      co.values_bytes = n * 4;
      co.values_off = RB.take(n * 4 + 32);
      cp.rowoff_off = P.scratch.take((uint64_t)r->n_batches * ((uint64_t)r->batch + 1) * 4 + 16);
    } else {
      co.offsets_off = RB.take((uint64_t)r->n_batches * ((uint64_t)r->batch + 1) * 4 + 16);
    }
    cp.chartot_off = (uint32_t)P.n_chartot_slots;
    P.n_chartot_slots += 2ull * r->n_batches;
    cp.lens_off = P.scratch.take(n * 4 + 16);
    cp.length = plan_stream(P, s, c.column_id, ORCGPU_S_LENGTH);
    cp.dictbytes_idx = P.new_scalar(0);  // total value bytes of the column (all batches) / dictionary bytes
    cp.dense_off = P.scratch.take(n * 8 + 16 + 8ull * 512);  // (+ the values in front of an entry point: at most a run's)
    const bool dict = t != ORCGPU_T_BINARY && is_dict_encoding(c);
    if (dict) {
      // string.rs:65-82: dictionary = DICTIONARY_DATA + LENGTH (dictionary_size entries, no PRESENT); keys = DATA
      cp.dict = plan_stream(P, s, c.column_id, ORCGPU_S_DICTIONARY_DATA);
      cp.data = plan_stream(P, s, c.column_id, ORCGPU_S_DATA);
      cp.dictn_idx = P.new_scalar(c.dictionary_size);
      cp.dictlens_off = P.scratch.take((uint64_t)c.dictionary_size * 8 + 16);
      cp.dictoff_off = P.scratch.take(((uint64_t)c.dictionary_size + 1) * 4 + 16);
      if (dout) {
        // the file's dictionary, entry for entry: its offsets are formed where they stay, its bytes are copied behind them
        co.dict_offsets_off = RB.take(((uint64_t)c.dictionary_size + 1) * 4 + 16);
        co.dict_values_off = RB.take(cp.dict.len_upper + ORC_PAD);
      }
      cp.dicttotal_idx = P.new_scalar(0);
      cp.job_length = add_job(P, vcls, class_codec(vcls), false, 64, 8, cp.length, cp.dictn_idx, c.dictionary_size, si, ci, ORCGPU_S_LENGTH);
      P.jobs[cp.job_length].out_scratch_off = cp.dictlens_off;
      // keys: decoded as the reference does (unsigned, 64 bit) but kept as narrow as the dictionary allows -- 1 byte for up
      // to 255 entries, 2 for up to 65 535, else 4 --, all ones for what cannot be a key (store_val): they are read twice more
      cp.key_bytes = c.dictionary_size <= 255 ? 1 : (c.dictionary_size <= 65535 ? 2 : 4);
      cp.job_data = add_job(P, vcls, class_codec(vcls), false, 64, (uint8_t)cp.key_bytes, cp.data, cp.nonnull_idx, n, si, ci, ORCGPU_S_DATA);
      P.jobs[cp.job_data].out_scratch_off = cp.dense_off;
      cp.dense_off += (uint64_t)cp.data.skip_values * cp.key_bytes;
      cp.is_dict = true;
      co.values_in_chars = !dout;
    } else {
      cp.data = plan_stream(P, s, c.column_id, ORCGPU_S_DATA);
      cp.job_length = add_job(P, vcls, class_codec(vcls), false, 64, 8, cp.length, cp.nonnull_idx, n, si, ci, ORCGPU_S_LENGTH);
      P.jobs[cp.job_length].out_scratch_off = cp.dense_off;
      cp.dense_off += 8ull * cp.length.skip_values;
      // (dictionary output of a DIRECT stripe: the identity dictionary -- the DATA bytes are its bytes, one entry per non-null row)
      uint64_t bytes_off = RB.take(cp.data.len_upper + ORC_PAD);
      if (dout) {
        co.dict_values_off = bytes_off;
        co.dict_offsets_off = RB.take((n + 1) * 4 + 16);
      } else {
        co.values_bytes = cp.data.len_upper;
        co.values_off = bytes_off;
      }
      cp.nonascii_idx = P.new_scalar(0);
      // a compressed DATA stream read from its first byte: decompressed where its bytes belong (lineitem's l_comment: 2 GB a step
      // that were written to the workspace, read again and written to the result)
      if (cp.data.exists && cp.data.scratch_off != ~0ull && cp.data.src && !cp.data.src->skip_bytes && !cp.data.skip_values) {
        for (size_t k = P.decomp.size(); k-- > 0;)
          if (P.decomp[k].st == cp.data.src && P.decomp[k].stripe == s) {
            P.decomp[k].result_index = cp.stripe;
            P.decomp[k].result_off = bytes_off;
            cp.data.in_result = true;
            break;
          }
      }
    }
    return ORCGPU_OK;
  }
  if (t == ORCGPU_T_LIST || t == ORCGPU_T_MAP) {
    // list.rs:63-87 / map.rs:74-104: LENGTH (unsigned RLE, one value per non-null row) -> per-batch int32 offsets restarting
    // at 0; what the lengths count -- the elements -- is decoded in a pass of its own once their total is known
    co.is_list = true;
    co.is_map = t == ORCGPU_T_MAP;
    co.offsets_off = RB.take((uint64_t)r->n_batches * ((uint64_t)r->batch + 1) * 4 + 16);
    cp.chartot_off = (uint32_t)P.n_chartot_slots;
    P.n_chartot_slots += 2ull * r->n_batches;
    cp.lens_off = P.scratch.take(n * 4 + 16);
    cp.length = plan_stream(P, s, c.column_id, ORCGPU_S_LENGTH);
    cp.dictbytes_idx = P.new_scalar(0);  // total elements of the column (all batches)
    cp.dense_off = P.scratch.take(n * 8 + 16 + 8ull * cp.length.skip_values);
    cp.job_length = add_job(P, vcls, class_codec(vcls), false, 64, 8, cp.length, cp.nonnull_idx, n, si, ci, ORCGPU_S_LENGTH);
    P.jobs[cp.job_length].out_scratch_off = cp.dense_off;
    cp.dense_off += 8ull * cp.length.skip_values;
    return ORCGPU_OK;
  }
  if (t == ORCGPU_T_DECIMAL) {
    cp.data = plan_stream(P, s, c.column_id, ORCGPU_S_DATA);
    cp.secondary = plan_stream(P, s, c.column_id, ORCGPU_S_SECONDARY);
    co.values_bytes = n * 16;
    co.values_off = RB.take(n * 16 + 16, 256);
    cp.dense_off = P.scratch.take(n * 16 + 16, 256);   // i128 dense values
    cp.dense2_off = P.scratch.take(n * 4 + 16 + 4ull * cp.secondary.skip_values);  // i32 dense scales
    cp.n_term_words = (cp.data.len_upper + 63) / 64;
    cp.tmask_off = P.scratch.take(cp.n_term_words * 8 + 16);
    cp.tpop_off = P.scratch.take(cp.n_term_words * 4 + 16);
    cp.trank_off = P.scratch.take(cp.n_term_words * 4 + 16);
    cp.ttiles_off = P.scratch.take(((cp.n_term_words + 1023) / 1024) * 4 + 16);
    cp.job_secondary = add_job(P, vcls, class_codec(vcls), true, 32, 4, cp.secondary, cp.nonnull_idx, n, si, ci, ORCGPU_S_SECONDARY);
    P.jobs[cp.job_secondary].out_scratch_off = cp.dense2_off;
    cp.dense2_off += 4ull * cp.secondary.skip_values;
    // a column without nulls (the varint decoder rescales and writes the Arrow buffer itself, launch_finish_ext): when the SECONDARY
    // stream turns out to hold nothing but the column's scale (rle2_uniform_kernel) it is not expanded and not read
    if (!cp.has_present && cp.n_term_words && !cp.secondary.skip_values && cp.secondary.exists && c.scale < 64) {
      cp.uniform_idx = P.new_scalar(0);
      P.jobs[cp.job_secondary].uniform_idx = cp.uniform_idx;
      P.jobs[cp.job_secondary].uniform_value = c.scale;
    }
    return ORCGPU_OK;
  }
  set_err(s->ctx, "column %u: ORC type kind %d not supported", c.column_id, t);
  return ORCGPU_UNSUPPORTED;
}

const uint8_t* plain_ptr(const PlainStream& ps, const uint8_t* S) { return ps.scratch_off != ~0ull ? S + ps.scratch_off : ps.dev; }

// phase 1 of the string / decimal finishers (everything that does not need the dictionary-gather output size)
// (nothing is launched here: the launches are filed in `fin` by pipeline stage and leave together, see FinBatch)
int launch_finish_ext(LaneRun& R, FinBatch& fin, ColPlan& cp, ColumnOut& co, orcgpu_result* r) {
  uint8_t* const S = R.S;
  uint64_t* const d_scalars = R.d_scalars;
  const uint64_t nr = cp.n_rows;
  const unsigned long long* vbits = R.vbits(cp);
  const uint32_t* rank = R.rank(cp);
  unsigned long long* err = reinterpret_cast<unsigned long long*>(d_scalars + cp.err_idx);
  const int t = cp.c.orc_type;
  if (is_string_type(t)) {
    int32_t* lens = reinterpret_cast<int32_t*>(S + cp.lens_off);
    uint8_t* const arena = R.arena(r);
    int32_t* offsets = reinterpret_cast<int32_t*>(cp.dict_out ? S + cp.rowoff_off : arena + co.offsets_off);
    unsigned long long* chartot = R.d_chartot + cp.chartot_off;
    unsigned long long* charbase = chartot + r->n_batches;
    const bool utf8 = t != ORCGPU_T_BINARY;
    if (cp.is_dict) {
      int32_t* doff = reinterpret_cast<int32_t*>(cp.dict_out ? arena + co.dict_offsets_off : S + cp.dictoff_off);
      const uint8_t* dbytes = plain_ptr(cp.dict, S);
      unsigned long long* derr = reinterpret_cast<unsigned long long*>(d_scalars + cp.dicterr_idx);
      fin.add<dict_offsets_body, 256>(0, 1, true, (const int64_t*)(S + cp.dictlens_off), (const uint64_t*)d_scalars, cp.dictn_idx,
                                      cp.dict.len_idx, doff, d_scalars + cp.dicttotal_idx, derr);
      if (utf8 && cp.dict.len_upper) {
        fin.add<utf8_validate_body, 256>(1, (cp.dict.len_upper + 15) / 16, false, dbytes, (const uint64_t*)d_scalars, cp.dicttotal_idx, cp.dict.len_idx, derr, (uint64_t*)nullptr);
        uint64_t dn = (uint64_t)cp.c.dictionary_size + 1;
        fin.add<utf8_boundaries_body, 256>(2, dn, false, dbytes, (const int32_t*)doff, (const unsigned long long*)nullptr,
                                           (const unsigned long long*)nullptr, dn, (uint32_t)std::min<uint64_t>(dn, 0xffffffffu), (const uint64_t*)d_scalars,
                                           cp.dicttotal_idx, cp.dict.len_idx, derr, (const uint64_t*)nullptr);
      }
      if (cp.dict_out) {
        // (the entries' bytes as they are; the keys follow behind the finishers: launch_dict_keys)
        if (cp.dict.len_upper) fin.add<copy_bytes_body, 256>(0, (cp.dict.len_upper + 15) / 16, false, dbytes, arena + co.dict_values_off, cp.dict.len_upper);
        return ORCGPU_OK;
      }
      // keys -> lengths -> offsets -> gather run for all dictionary columns of the call together: launch_dict_rows
      R.P.pending_gathers.push_back((int)(&cp - R.P.cols.data()));
      return ORCGPU_OK;
    } else {
      // charbase (still zero from the summary upload) collects the out-of-range lengths until batch_base_kernel fills it
      fin.add<string_lens_body, 256>(0, nr, false, (const int64_t*)(S + cp.dense_off), vbits, rank, lens, nr, r->batch, charbase, err);
      fin.add<batch_offsets_body, 256>(1, (uint64_t)r->n_batches, true, (const int32_t*)lens, nr, r->batch, offsets, chartot,
                                       (const unsigned long long*)charbase, err, (uint32_t)ORC_E_OFFSET_OVERFLOW);
    }
    fin.add<batch_base_body, 256>(2, 1, true, (const unsigned long long*)chartot, charbase, r->n_batches, d_scalars + cp.dictbytes_idx);
    if (!cp.is_dict) {
      uint8_t* values = arena + (cp.dict_out ? co.dict_values_off : co.values_off);
      const uint8_t* src = cp.data.in_result ? values : plain_ptr(cp.data, S);
      fin.add<string_data_check_body, 64>(3, (uint64_t)(r->n_batches + 63) / 64, true, (const unsigned long long*)chartot,
                                          (const unsigned long long*)charbase, r->n_batches, (const uint64_t*)d_scalars, cp.data.len_idx, r->batch, err);
      if (cp.data.len_upper) {
        unsigned long long* uerr = reinterpret_cast<unsigned long long*>(d_scalars + cp.utf8err_idx);
        if (cp.data.in_result) {
          // (the bytes are where they belong: text is only checked)
          if (utf8) fin.add<utf8_validate_body, 256>(3, (cp.data.len_upper + 15) / 16, false, src, (const uint64_t*)d_scalars, cp.dictbytes_idx, cp.data.len_idx, uerr, d_scalars + cp.nonascii_idx);
        } else if (utf8) fin.add<copy_validate_body, 256>(3, (cp.data.len_upper + 15) / 16, false, src, values, cp.data.len_upper, (const uint64_t*)d_scalars, cp.dictbytes_idx, cp.data.len_idx, uerr, d_scalars + cp.nonascii_idx);
        else fin.add<copy_bytes_body, 256>(3, (cp.data.len_upper + 15) / 16, false, src, values, cp.data.len_upper);
        if (utf8) {
          fin.add<utf8_boundaries_body, 256>(5, nr, false, (const uint8_t*)values, (const int32_t*)offsets, (const unsigned long long*)charbase,
                                             (const unsigned long long*)chartot, nr, r->batch, (const uint64_t*)d_scalars, cp.dictbytes_idx,
                                             cp.data.len_idx, err, (const uint64_t*)(d_scalars + cp.nonascii_idx));
        }
      }
    }
    return ORCGPU_OK;
  }
  if (t == ORCGPU_T_LIST || t == ORCGPU_T_MAP) {
    int32_t* lens = reinterpret_cast<int32_t*>(S + cp.lens_off);
    int32_t* offsets = reinterpret_cast<int32_t*>(R.arena(r) + co.offsets_off);
    unsigned long long* chartot = R.d_chartot + cp.chartot_off;
    unsigned long long* charbase = chartot + r->n_batches;
    // (the same three steps as a direct string's lengths: spaced lengths, per-batch offsets and totals, their scan)
    fin.add<string_lens_body, 256>(0, nr, false, (const int64_t*)(S + cp.dense_off), vbits, rank, lens, nr, r->batch, charbase, err);
    fin.add<batch_offsets_body, 256>(1, (uint64_t)r->n_batches, true, (const int32_t*)lens, nr, r->batch, offsets, chartot,
                                     (const unsigned long long*)charbase, err, (uint32_t)ORC_E_ARROW);
    fin.add<batch_base_body, 256>(2, 1, true, (const unsigned long long*)chartot, charbase, r->n_batches, d_scalars + cp.dictbytes_idx);
    return ORCGPU_OK;
  }
  if (t == ORCGPU_T_DECIMAL) {
    const uint8_t* src = plain_ptr(cp.data, S);
    unsigned long long* tmask = reinterpret_cast<unsigned long long*>(S + cp.tmask_off);
    uint32_t* tpop = reinterpret_cast<uint32_t*>(S + cp.tpop_off);
    uint32_t* trank = reinterpret_cast<uint32_t*>(S + cp.trank_off);
    uint32_t* ttiles = reinterpret_cast<uint32_t*>(S + cp.ttiles_off);
    __int128* dense = reinterpret_cast<__int128*>(S + cp.dense_off);
    // (value-indexed error word, like the varint decoder's: the batch holding the first non-null row fails)
    fin.add<varint_empty_check_body, 64>(0, 1, true, (const uint64_t*)d_scalars, cp.data.len_idx, cp.nonnull_idx,
                                         reinterpret_cast<unsigned long long*>(d_scalars + cp.utf8err_idx));
    if (cp.n_term_words) {
      uint64_t ntiles = (cp.n_term_words + 1023) / 1024;
      fin.add<varint_terms_body, 256>(0, cp.n_term_words, false, src, (const uint64_t*)d_scalars, cp.data.len_idx, cp.n_term_words, tmask, tpop);
      fin.add<scan_tiles_body, 256>(1, ntiles, true, (const uint32_t*)tpop, trank, ttiles, cp.n_term_words);
      fin.add<scan_sums_body, 256>(2, 1, true, ttiles, ntiles, (uint64_t*)nullptr);
      fin.add<scan_apply_body, 256>(3, cp.n_term_words, false, trank, (const uint32_t*)ttiles, cp.n_term_words);
      // a column without nulls: value k is row k -- the varint decoder brings it to the column's scale and writes the Arrow buffer
      // itself (no decimal_finish pass: 36 bytes per value that re-read what was just written)
      const bool fused = !vbits && nr;
      __int128* const arrow = reinterpret_cast<__int128*>(R.arena(r) + co.values_off);
      fin.add<varint_decode128_body, 256>(4, (cp.data.len_upper + 7) / 8, false, src, (const uint64_t*)d_scalars, cp.data.len_idx, cp.nonnull_idx,
                                          (const unsigned long long*)tmask, (const uint32_t*)trank, fused ? arrow : dense, cp.data.len_upper,
                                          reinterpret_cast<unsigned long long*>(d_scalars + cp.utf8err_idx),
                                          fused ? (const int32_t*)(S + cp.dense2_off) : (const int32_t*)nullptr, (uint32_t)cp.c.scale,
                                          fused && cp.uniform_idx ? (const uint64_t*)(d_scalars + cp.uniform_idx) : (const uint64_t*)nullptr);
      if (fused) return ORCGPU_OK;
    }
    fin.add<decimal_finish_body, 256>(5, nr, false, (const __int128*)dense, (const int32_t*)(S + cp.dense2_off), vbits, rank,
                                      reinterpret_cast<__int128*>(R.arena(r) + co.values_off), nr, cp.c.scale);
    return ORCGPU_OK;
  }
  return ORCGPU_OK;
}

// Dictionary output (ORCGPU_ARROW_DICTIONARY_UTF8), behind the finishers: one launch per column writes the stripe's int32 keys.
// A DICTIONARY stripe: the DATA ids, spaced over the rows and bounds-checked against the dictionary size on the device.  A
// DIRECT stripe: a valid row's rank among the valid rows, and with it entry `rank` of the identity dictionary's offsets.
// Nothing is sized on the host: keys and dictionary lie in the result's arena, at places known when the call was planned.
int launch_dict_keys(LaneRun& R) {
  uint8_t* const S = R.S;
  uint64_t* const d_scalars = R.d_scalars;
  for (auto& cp : R.P.cols) {
    if (cp.col < 0 || !cp.dict_out || !cp.n_rows) continue;
    orcgpu_result* r = R.P.results[cp.stripe];
    ColumnOut& co = r->cols[cp.col];
    uint8_t* const arena = R.arena(r);
    DictKeysJob j{};
    j.dense = cp.is_dict ? S + cp.dense_off : nullptr;
    j.vbits = R.vbits(cp);
    j.rank = R.rank(cp);
    j.keys = reinterpret_cast<int32_t*>(arena + co.values_off);
    j.err = reinterpret_cast<unsigned long long*>(d_scalars + cp.err_idx);
    j.dict_err = reinterpret_cast<const unsigned long long*>(d_scalars + cp.dicterr_idx);
    j.scalars = d_scalars;
    j.n_rows = cp.n_rows;
    j.batch = r->batch;
    j.key_bytes = cp.key_bytes;
    j.dict_n_idx = cp.dictn_idx;
    if (!cp.is_dict) {
      j.row_offsets = reinterpret_cast<const int32_t*>(S + cp.rowoff_off);
      j.charbase = R.d_chartot + cp.chartot_off + r->n_batches;
      j.dict_off = reinterpret_cast<int32_t*>(arena + co.dict_offsets_off);
      j.nonnull_idx = cp.nonnull_idx;
      j.total_idx = cp.dictbytes_idx;
    }
    HIP_TRY(R.ctx, launch(dict_keys_kernel, (cp.n_rows + DICT_PER - 1) / DICT_PER, false, 256, R.st, j));
  }
  return ORCGPU_OK;
}

// Dictionary columns, pass 1: one descriptor per column, ONE launch for the per-batch value byte totals (keys bounds-checked)
// and one for their scan per column.
int launch_dict_rows(LaneRun& R) {
  Plan& P = R.P;
  if (P.pending_gathers.empty()) return ORCGPU_OK;
  orcgpu_ctx* const ctx = R.ctx;
  hipStream_t st = R.st;
  uint8_t* const S = R.S;
  uint64_t* const d_scalars = R.d_scalars;
  P.dictjobs.clear();
  uint32_t max_batches = 0;
  for (int idx : P.pending_gathers) {
    ColPlan& cp = P.cols[idx];
    orcgpu_result* r = P.results[cp.stripe];
    ColumnOut& co = r->cols[cp.col];
    DictJob j{};
    j.dense = S + cp.dense_off;
    j.vbits = R.vbits(cp);
    j.rank = R.rank(cp);
    j.doff = reinterpret_cast<const int32_t*>(S + cp.dictoff_off);
    j.dbytes = plain_ptr(cp.dict, S);
    j.offsets = reinterpret_cast<int32_t*>(R.arena(r) + co.offsets_off);
    j.chartot = R.d_chartot + cp.chartot_off;
    j.err = reinterpret_cast<unsigned long long*>(d_scalars + cp.err_idx);
    j.dict_err = reinterpret_cast<const unsigned long long*>(d_scalars + cp.dicterr_idx);
    j.out_chars = nullptr;
    j.total_out = d_scalars + cp.dictbytes_idx;
    j.n_rows = cp.n_rows;
    j.batch = r->batch;
    j.n_batches = r->n_batches;
    j.dict_n_idx = cp.dictn_idx;
    j.key_bytes = cp.key_bytes;
    P.dictjobs.push_back(j);
    max_batches = std::max(max_batches, r->n_batches);
  }
  DictJob* d_jobs = reinterpret_cast<DictJob*>(S + P.dictjobs_off);
  const uint32_t n = (uint32_t)P.dictjobs.size();
  HIP_TRY(ctx, ctx->upload(d_jobs, P.dictjobs.data(), n * sizeof(DictJob), st));
  if (max_batches) {
    for (uint32_t o = 0; o < n; o += 65535u)  // grid.y limit
      hipLaunchKernelGGL(dict_totals_kernel, dim3(max_batches, std::min<uint32_t>(65535u, n - o)), dim3(256), 0, st, (const DictJob*)(d_jobs + o),
                         (const uint64_t*)d_scalars);
    HIP_TRY(ctx, hipGetLastError());
  }
  HIP_TRY(ctx, launch(dict_base_kernel, (uint64_t)n, true, 256, st, (const DictJob*)d_jobs));
  return ORCGPU_OK;
}

// pass 2: offsets and value bytes of the dictionary columns.  The character arenas are sized exactly from the totals of pass 1.
// A result that has been decoded into before has its arena from then: the columns are placed in it on the device
// (dict_place_kernel), the host does not wait for the totals, and settle_dict_places() -- behind the call's closing
// synchronisation -- places them the same way, or sends pass 2 again if the arena was too small.  A fresh result costs one small
// D2H + sync here (the only one inside a decode call).
static void place_dict_columns(Plan& P, const uint64_t* h_scalars, std::vector<uint64_t>& need) {
  need.assign(P.results.size(), 0);
  for (int idx : P.pending_gathers) {
    ColPlan& cp = P.cols[idx];
    ColumnOut& co = P.results[cp.stripe]->cols[cp.col];
    uint64_t total = h_scalars[cp.dictbytes_idx];
    co.values_off = align_up(need[cp.stripe]);
    co.values_bytes = total;
    need[cp.stripe] = co.values_off + total + ORC_PAD;
  }
}
static int launch_dict_emit(LaneRun& R, bool upload) {
  Plan& P = R.P;
  orcgpu_ctx* const ctx = R.ctx;
  uint32_t max_batches = 0;
  for (size_t k = 0; k < P.pending_gathers.size(); k++) {
    ColPlan& cp = P.cols[P.pending_gathers[k]];
    orcgpu_result* r = P.results[cp.stripe];
    ColumnOut& co = r->cols[cp.col];
    if (upload) P.dictjobs[k].out_chars = co.values_bytes ? r->chars[ctx->lane_id].p + co.values_off : nullptr;
    max_batches = std::max(max_batches, r->n_batches);  // (offsets are written for every column, value bytes or not)
  }
  if (max_batches) {
    hipStream_t st = R.st;
    DictJob* d_jobs = reinterpret_cast<DictJob*>(R.S + P.dictjobs_off);
    const uint32_t n = (uint32_t)P.dictjobs.size();
    if (upload) HIP_TRY(ctx, ctx->upload(d_jobs, P.dictjobs.data(), n * sizeof(DictJob), st));
    HIP_TRY(ctx, hipEventRecord(ctx->kev[1][0], st));
    for (uint32_t o = 0; o < n; o += 65535u)  // grid.y limit
      hipLaunchKernelGGL(dict_emit_kernel, dim3(max_batches, std::min<uint32_t>(65535u, n - o)), dim3(256), 0, st, (const DictJob*)(d_jobs + o), (const uint64_t*)R.d_scalars);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->kev[1][1], st));
    ctx->kev_used[1] = true;
  }
  return ORCGPU_OK;
}
int launch_post_ext(LaneRun& R) {
  Plan& P = R.P;
  orcgpu_ctx* const ctx = R.ctx;
  uint8_t* const S = R.S;
  P.dictplaces.clear();
  P.dictplace_result.clear();
  if (P.pending_gathers.empty()) return ORCGPU_OK;
  hipStream_t st = R.st;
  // the results' arenas as they are: usable when every result has one and its columns follow one another in the job table
  constexpr bool never = false;
  bool on_device = !never;
  for (size_t k = 0; k < P.pending_gathers.size() && on_device; k++) {
    const uint32_t si = (uint32_t)P.cols[P.pending_gathers[k]].stripe;
    if (!P.dictplace_result.empty() && P.dictplace_result.back() == si) {
      P.dictplaces.back().count++;
      continue;
    }
    const DevBuf& C = P.results[si]->chars[ctx->lane_id];
    on_device = C.cap > 0 && std::find(P.dictplace_result.begin(), P.dictplace_result.end(), si) == P.dictplace_result.end();
    P.dictplaces.push_back(DictPlace{C.p, C.cap, (uint32_t)k, 1});
    P.dictplace_result.push_back(si);
  }
  if (on_device) {
    const uint32_t np = (uint32_t)P.dictplaces.size();
    DictPlace* d_places = reinterpret_cast<DictPlace*>(S + P.dictplaces_off);
    HIP_TRY(ctx, ctx->upload(d_places, P.dictplaces.data(), np * sizeof(DictPlace), st));
    HIP_TRY(ctx, launch(dict_place_kernel, (uint64_t)np, false, 64, st, reinterpret_cast<DictJob*>(S + P.dictjobs_off), (const DictPlace*)d_places, np, (uint64_t)ORC_PAD,
                        (uint64_t)kAlign));
    return launch_dict_emit(R, false);
  }
  P.dictplaces.clear();
  P.dictplace_result.clear();
  HIP_TRY(ctx, launch(summary_to_host_kernel, (uint64_t)P.scalars.size(), false, 256, st, (const unsigned long long*)(R.dsum + R.SL.scalars_off),
                      (unsigned long long*)(R.hs + R.SL.scalars_off), (uint64_t)P.scalars.size()));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  std::vector<uint64_t> need;
  place_dict_columns(P, R.h_scalars(), need);
  for (size_t si = 0; si < P.results.size(); si++) {
    P.results[si]->chars_used[ctx->lane_id] = need[si];
    if (need[si] && !P.results[si]->chars[ctx->lane_id].ensure(need[si] + kAlign)) {
      set_err(ctx, "hipMalloc(%llu) for dictionary string values failed", (unsigned long long)need[si]);
      return ORCGPU_HIP_ERROR;
    }
  }
  return launch_dict_emit(R, true);
}

// Behind the call's closing synchronisation: where the device placed the dictionary columns' value bytes (see launch_post_ext).
int settle_dict_places(LaneRun& R) {
  Plan& P = R.P;
  orcgpu_ctx* const ctx = R.ctx;
  if (P.dictplaces.empty()) return ORCGPU_OK;
  std::vector<uint64_t> need;
  place_dict_columns(P, R.h_scalars(), need);
  bool again = false;
  for (size_t k = 0; k < P.dictplaces.size(); k++) again = again || need[P.dictplace_result[k]] + kAlign > P.dictplaces[k].cap;
  for (size_t si = 0; si < P.results.size(); si++) {
    P.results[si]->chars_used[ctx->lane_id] = need[si];
    if (again && need[si] && !P.results[si]->chars[ctx->lane_id].ensure(need[si] + kAlign)) {
      set_err(ctx, "hipMalloc(%llu) for dictionary string values failed", (unsigned long long)need[si]);
      return ORCGPU_HIP_ERROR;
    }
  }
  if (!again) return ORCGPU_OK;
  // (every column once more: the arenas that grew are new memory)
  int rc = launch_dict_emit(R, true);
  if (rc) return rc;
  HIP_TRY(ctx, hipStreamSynchronize(R.st));
  return ORCGPU_OK;
}

template <typename F>
uint32_t resolve_job_batch(const ColPlan& cp, int k, uint64_t idx, F& batch_of_dense) {
  // the dictionary LENGTH stream is decoded when the column decoder is built: a failure there fails
  // the whole stripe (new_string_decoder, string.rs:70-72), i.e. batch 0
  if (k == 2 && cp.is_dict) return 0;
  return batch_of_dense(idx);
}

template <typename F>
void resolve_ext(LaneRun& R, ColPlan& cp, ColumnOut& co, orcgpu_result* r, F& consider) {
  const uint64_t* h_scalars = R.h_scalars();
  const unsigned long long* h_chartot = R.h_chartot();
  const int t = cp.c.orc_type;
  if ((t == ORCGPU_T_LIST || t == ORCGPU_T_MAP) && cp.n_rows) {
    co.char_total.assign(h_chartot + cp.chartot_off, h_chartot + cp.chartot_off + r->n_batches);
    co.char_base.assign(h_chartot + cp.chartot_off + r->n_batches, h_chartot + cp.chartot_off + 2ull * r->n_batches);
  } else if (is_string_type(t) && cp.n_rows) {
    co.char_total.assign(h_chartot + cp.chartot_off, h_chartot + cp.chartot_off + r->n_batches);
    co.char_base.assign(h_chartot + cp.chartot_off + r->n_batches, h_chartot + cp.chartot_off + 2ull * r->n_batches);
    if (cp.dict_out) {
      uint64_t nulls = 0;
      for (auto v : co.null_counts) nulls += v;
      co.dict_len = cp.is_dict ? cp.c.dictionary_size : cp.n_rows - nulls;
      co.dict_bytes = std::min<uint64_t>(h_scalars[cp.is_dict ? cp.dicttotal_idx : cp.dictbytes_idx], 0x7fffffffull);
    }
    if (cp.is_dict) {
      unsigned long long de = h_scalars[cp.dicterr_idx];
      if (de != RLE_NO_ERR) consider((int)ORC_E_ARROW == (int)(de & 0xff) ? ORCGPU_ARROW : (int)(de & 0xff), 0u);
    } else {
      unsigned long long ue = h_scalars[cp.utf8err_idx];
      if (ue != RLE_NO_ERR) {
        // invalid byte position -> the batch whose value bytes contain it
        uint64_t pos = ue >> 8;
        uint32_t b = 0;
        while (b + 1 < r->n_batches && co.char_base[b + 1] <= pos) b++;
        consider((int)(ue & 0xff), b);
      }
    }
  } else if (t == ORCGPU_T_DECIMAL && cp.n_rows) {
    unsigned long long ve = h_scalars[cp.utf8err_idx];  // varint error: dense value index
    if (ve != RLE_NO_ERR) {
      uint64_t d = ve >> 8, acc = 0;
      uint32_t b = 0;
      for (; b < r->n_batches; b++) {
        uint64_t rows = std::min<uint64_t>(r->batch, r->n_rows - (uint64_t)b * r->batch);
        acc += rows - co.null_counts[b];
        if (d < acc) break;
      }
      consider((int)(ve & 0xff), std::min<uint32_t>(b, r->n_batches ? r->n_batches - 1 : 0));
    }
  }
}

uint64_t result_column_bytes(const orcgpu_result* r, const ColumnOut& co) {
  uint64_t b = 0;
  if (co.is_list) {
    b += (uint64_t)r->n_batches * 4 + r->n_rows * 4;  // offsets (the elements are counted by their own result)
  } else if (co.is_string) {
    for (auto v : co.char_total) b += v;
    b += (uint64_t)r->n_batches * 4 + r->n_rows * 4;
  } else if (co.is_bool) {
    b += (r->n_rows + 7) / 8;
  } else {
    b += co.values_bytes;
    if (co.dict_out) b += (co.dict_len + 1) * 4 + co.dict_bytes;  // the stripe's dictionary, once
  }
  for (uint32_t i = 0; i < r->n_batches; i++)
    if (co.null_counts[i]) b += (std::min<uint64_t>(r->batch, r->n_rows - (uint64_t)i * r->batch) + 7) / 8;
  return b;
}

}  // namespace
