// orcgpu_writer_flush.inc -- a stripe of the ArrowWriter (orcgpu_writer.inc) flushed: which string columns get a dictionary
// (wr_dictionaries), then StripeWriter::finish_stripe (wr_flush) in its steps -- the row index statistics enqueued, every
// stream of every column enqueued from its description (orcgpu_writer_host.inc: wr_streams), compression, the ROW_INDEX streams
// assembled on the host (and the BLOOM_FILTER_UTF8 streams around the bitsets the device built), the streams packed and copied
// back, the footer written.
namespace {

// Which string columns of the stripe being flushed are written DICTIONARY_V2 (orcgpu_writer_set_dictionary), and their
// dictionaries.  Every such column's tables are enqueued (device/writer_dict.hip), then one wait, whatever the column count,
// brings back each column's entries d and their bytes; a column goes DICTIONARY_V2 iff (double)d <= threshold * (double)n.
int wr_dictionaries(orcgpu_writer* w) {
  orcgpu_ctx* ctx = w->ctx;
  hipStream_t st = ctx->stream;
  std::vector<size_t> dc;
  for (size_t ci = 0; ci < w->cols.size(); ci++) {
    WrCol& c = w->cols[ci];
    c.dict = false;
    c.dict_size = c.dict_bytes = 0;
    if (w->dict_threshold > 0 && c.is_utf8() && c.n_valid) dc.push_back(ci);
  }
  if (dc.empty()) return ORCGPU_OK;
  const uint64_t K = dc.size();
  if (!wr_ensure(w, w->dict_res, (2 * K + 1) * 8 + kAlign)) return ORCGPU_HIP_ERROR;
  uint64_t* d_res = (uint64_t*)w->dict_res.p;  // [column] entries, bytes; then `bad`
  uint32_t* d_bad = (uint32_t*)(d_res + 2 * K);
  WR_TRY(hipMemsetAsync(d_bad, 0, 8, st));
  for (uint64_t k = 0; k < K; k++) {
    WrCol& c = w->cols[dc[k]];
    WrColDev& d = w->dev[dc[k]];
    const uint64_t n = c.n_valid;
    if (n >= 0x7fffffffull) {
      set_err(ctx, "writer: %llu strings of column %zu in one stripe (fewer than 2^31 with a dictionary threshold)", (unsigned long long)n, dc[k]);
      return ORCGPU_INVALID_ARGUMENT;
    }
    uint64_t slots = 64;
    while (slots < 2 * n) slots <<= 1;
    Bump T;
    const uint64_t o_len32 = T.take(n * 4), o_offs = T.take(n * 8), o_sums = T.take((n / 2048 + 2) * 8), o_tot = T.take(16), o_table = T.take(slots * 8),
                   o_slot = T.take(n * 4), o_flag = T.take(n * 4), o_flen = T.take(n * 4), o_first = T.take(n * 8), o_foff = T.take(n * 8), o_d = T.take(16),
                   o_D = T.take(16), o_erow = T.take(n * 4), o_eoff = T.take(n * 8);
    d.o_dict_ids = T.take(n * (uint64_t)c.elem);
    d.o_dict_len = T.take(n * (uint64_t)c.elem);
    d.o_dict_data = T.take(align_up(c.n_bytes, 16) + 16);
    if (!wr_ensure(w, d.b_dict, T.off + kAlign)) {
      set_err(ctx, "writer: out of device memory (%llu bytes of dictionary tables)", (unsigned long long)T.off);
      return ORCGPU_HIP_ERROR;
    }
    uint8_t* t = d.b_dict.p;
    uint32_t *len32 = (uint32_t*)(t + o_len32), *rep = (uint32_t*)(t + o_table), *low = rep + slots, *slot_of = (uint32_t*)(t + o_slot),
             *flag = (uint32_t*)(t + o_flag), *flen = (uint32_t*)(t + o_flen), *erow = (uint32_t*)(t + o_erow);
    uint64_t *offs = (uint64_t*)(t + o_offs), *sums = (uint64_t*)(t + o_sums), *first = (uint64_t*)(t + o_first), *foff = (uint64_t*)(t + o_foff),
             *tot_d = (uint64_t*)(t + o_d), *tot_D = (uint64_t*)(t + o_D), *eoff = (uint64_t*)(t + o_eoff);
    WR_TRY(launch(wd_len32_kernel, n, false, 256, st, (const void*)d.vals.p, c.elem, n, len32));
    int rc = enc_scan(ctx, st, len32, n, sums, (uint64_t*)(t + o_tot), offs);
    if (rc) return rc;
    WR_TRY(hipMemsetAsync(rep, 0xff, slots * 8, st));
    WR_TRY(launch(wd_insert_kernel, n, false, 256, st, (const uint8_t*)d.data.p, (const uint64_t*)offs, (const uint32_t*)len32, (uint32_t)n, rep, low,
                  (uint32_t)(slots - 1), w->dict_hash_mask, slot_of, d_bad));
    WR_TRY(launch(wd_flag_kernel, n, false, 256, st, (const uint32_t*)slot_of, (const uint32_t*)low, (const uint32_t*)len32, (uint32_t)n, flag, flen));
    rc = enc_scan(ctx, st, flag, n, sums, tot_d, first);
    if (rc) return rc;
    rc = enc_scan(ctx, st, flen, n, sums, tot_D, foff);
    if (rc) return rc;
    WR_TRY(launch(wd_ids_kernel, n, false, 256, st, (const uint32_t*)slot_of, (const uint32_t*)low, (const uint32_t*)flag, (const uint64_t*)first,
                  (const uint64_t*)foff, (const uint32_t*)len32, (uint32_t)n, c.elem, (void*)(t + d.o_dict_ids), (void*)(t + d.o_dict_len), erow, eoff, d_bad));
    WR_TRY(launch(wd_gather_kernel, (c.n_bytes + 15) / 16, false, 256, st, (const uint8_t*)d.data.p, (const uint64_t*)offs, (const uint32_t*)erow,
                  (const uint64_t*)eoff, (const uint64_t*)tot_d, (const uint64_t*)tot_D, (uint4*)(t + d.o_dict_data)));
    WR_TRY(hipMemcpyAsync(d_res + 2 * k, tot_d, 8, hipMemcpyDeviceToDevice, st));
    WR_TRY(hipMemcpyAsync(d_res + 2 * k + 1, tot_D, 8, hipMemcpyDeviceToDevice, st));
  }
  std::vector<uint64_t> res(2 * K + 1, 0);
  WR_TRY(hipMemcpyAsync(res.data(), d_res, (2 * K + 1) * 8, hipMemcpyDeviceToHost, st));
  int rc = wr_sync(w);
  if (rc) return rc;
  if ((uint32_t)res[2 * K]) {
    set_err(ctx, "writer: a string found no slot in its column's dictionary table");
    return ORCGPU_UNEXPECTED;
  }
  for (uint64_t k = 0; k < K; k++) {
    WrCol& c = w->cols[dc[k]];
    const uint64_t n_entries = res[2 * k];
    if (n_entries > c.n_valid || res[2 * k + 1] > c.n_bytes) return ORCGPU_UNEXPECTED;
    if ((double)n_entries <= w->dict_threshold * (double)c.n_valid) {
      c.dict = true;
      c.dict_size = n_entries;
      c.dict_bytes = res[2 * k + 1];
    }
  }
  return ORCGPU_OK;
}

// what the steps of a flush hand on
struct WrFlush {
  uint64_t n_streams = 0;
  std::vector<WrStreamOut> streams;  // in the stripe's stream order
  std::vector<uint64_t> known;       // a stream's length where the host knows it (~0: it comes back from the device)
  std::vector<uint64_t> lens, zslot;  // the streams' lengths in the file; compressed: their slots in zout
  uint64_t at = 0;                   // the end of the last slot of w->slots
  uint64_t total = 0;                // the streams' bytes
  bool comp = false;
  // row index: groups of S rows, G of them, NJ (column, group) jobs; the tables' places in w->ix, brought back from o_recs on
  uint64_t S = 0, G = 0, NJ = 0;
  uint64_t o_vscan = 0, o_bscan = 0, o_recs = 0, o_pos = 0, o_side = 0, ix_span = 0;
  uint64_t o_bloom = 0;  // Bloom filters: the listed columns' bitsets, [listed column][group][words], brought back with the records
  std::vector<std::vector<std::pair<uint64_t, int>>> ix_streams;  // a column's streams (index, position form), PRESENT, DATA, LENGTH
  std::vector<std::vector<uint8_t>> index;                         // the ROW_INDEX streams, column 0 first
  std::vector<std::vector<uint8_t>> bloom;                         // the BLOOM_FILTER_UTF8 streams, [column id] (empty: none)
};

// room: the lengths, the bitmaps of the Boolean / PRESENT streams
int wr_flush_room(orcgpu_writer* w, WrFlush& F) {
  uint64_t bits_room = 0;
  for (auto& c : w->cols) {
    WrStream s[WR_MAX_STREAMS];
    const int ns = wr_streams(c, wr_counts(c), false, s);
    F.n_streams += ns;
    for (int i = 0; i < ns; i++)
      if (s[i].enc == WR_ENC_BITS) bits_room += align_up(2 * wr_bits_bytes(s[i].n) + 16);
  }
  if (!wr_ensure(w, w->lens, F.n_streams * 8 + kAlign) || !wr_ensure(w, w->bits, bits_room + kAlign)) return ORCGPU_HIP_ERROR;
  w->bits_at = 0;
  F.known.assign(F.n_streams, ~0ull);
  return ORCGPU_OK;
}

// row index: the groups' statistics, enqueued ahead of the streams (jobs: column * G + group)
int wr_flush_stats(orcgpu_writer* w, WrFlush& F) {
  orcgpu_ctx* ctx = w->ctx;
  const size_t nc = w->cols.size();
  const uint64_t S = F.S, G = F.G, NJ = F.NJ;
  if (NJ >= 0x7fffffffull) {
    set_err(ctx, "writer: %llu row groups in one stripe (fewer than 2^31)", (unsigned long long)NJ);
    return ORCGPU_INVALID_ARGUMENT;
  }
  uint64_t side_bound = 0;
  for (auto& c : w->cols)
    if (c.is_utf8()) side_bound += std::min<uint64_t>(2ull * IX_STR_KEEP * G, 2 * c.n_bytes);
  Bump X;
  const uint64_t o_cols = X.take(nc * sizeof(IxCol)), o_cnt = X.take(NJ * 8);
  F.o_vscan = X.take((NJ + 1) * 8);
  const uint64_t o_blen = X.take(NJ * 8);
  F.o_bscan = X.take((NJ + 1) * 8);
  const uint64_t o_slen = X.take(NJ * 8), o_soff = X.take((NJ + 1) * 8);
  F.o_recs = X.take(NJ * sizeof(IxRec));  // (from here on: brought back)
  F.o_pos = X.take(F.n_streams * G * 32);
  F.o_side = X.take(side_bound);
  const uint64_t bloom_group = w->bloom_words * 8, bloom_col = G * bloom_group;  // bytes of a group's bitset, of a column's
  F.o_bloom = X.take(w->n_bloom * bloom_col);
  F.ix_span = X.off - F.o_recs;
  if (!wr_reserve(w, w->ix, X.off + kAlign, 0)) {
    set_err(ctx, "writer: out of device memory (%llu bytes of row index)", (unsigned long long)X.off);
    return ORCGPU_HIP_ERROR;
  }
  int rc = wr_pinned(w, w->ix_pinned, w->ix_pinned_cap, F.ix_span, false);
  if (rc) return rc;
  uint8_t* x = w->ix.p;
  IxCol* d_cols = (IxCol*)(x + o_cols);
  for (uint32_t i0 = 0; i0 < nc; i0 += IX_COLS_PER_ARG) {
    IxColArgs a{};
    a.at = i0;
    a.n = std::min<uint32_t>(IX_COLS_PER_ARG, (uint32_t)nc - i0);
    for (uint32_t i = 0; i < a.n; i++) {
      const WrCol& c = w->cols[i0 + i];
      const WrColDev& d = w->dev[i0 + i];
      a.c[i] = IxCol{d.pres.p, d.vals.p, d.src(wr_stats_src(c)), c.stream_kind, c.elem, c.is_utf8(), 0};
    }
    WR_TRY(launch(ix_put_cols_kernel, (uint64_t)1, true, 64, ctx->stream, a, d_cols));
  }
  uint64_t *d_cnt = (uint64_t*)(x + o_cnt), *d_vscan = (uint64_t*)(x + F.o_vscan), *d_blen = (uint64_t*)(x + o_blen), *d_bscan = (uint64_t*)(x + F.o_bscan),
           *d_slen = (uint64_t*)(x + o_slen), *d_soff = (uint64_t*)(x + o_soff);
  IxRec* d_recs = (IxRec*)(x + F.o_recs);
  const IxCol* cc = d_cols;
  WR_TRY(launch(ix_count_kernel, NJ, true, 256, ctx->stream, cc, w->rows, S, G, d_cnt));
  WR_TRY(launch(ix_scan_kernel, (uint64_t)1, true, 1024, ctx->stream, (const uint64_t*)d_cnt, NJ, d_vscan));
  WR_TRY(launch(ix_bytes_kernel, NJ, true, 256, ctx->stream, cc, G, (const uint64_t*)d_cnt, (const uint64_t*)d_vscan, d_blen));
  WR_TRY(launch(ix_scan_kernel, (uint64_t)1, true, 1024, ctx->stream, (const uint64_t*)d_blen, NJ, d_bscan));
  WR_TRY(launch(ix_stats_kernel, NJ, true, 256, ctx->stream, cc, w->rows, S, G, (const uint64_t*)d_cnt, (const uint64_t*)d_vscan, (const uint64_t*)d_bscan,
                d_recs, d_slen));
  WR_TRY(launch(ix_scan_kernel, (uint64_t)1, true, 1024, ctx->stream, (const uint64_t*)d_slen, NJ, d_soff));
  WR_TRY(launch(ix_side_kernel, NJ, true, 256, ctx->stream, cc, G, (const uint64_t*)d_soff, d_recs, x + F.o_side));
  // Bloom filters: a launch per listed column, a block per row group, over the tables just made.  A bitset that fits
  // BLOOM_LDS_BYTES is built in LDS; a larger one in its place, zeroed first
  uint64_t nb = 0;
  for (size_t ci = 0; ci < nc; ci++) {
    if (!w->cols[ci].bloom) continue;
    uint32_t* d_bits = (uint32_t*)(x + F.o_bloom + nb++ * bloom_col);
    if (bloom_group <= BLOOM_LDS_BYTES) {
      hipLaunchKernelGGL(bloom_lds_kernel, dim3((uint32_t)G), dim3(256), (uint32_t)bloom_group, ctx->stream, cc, (uint32_t)ci, G, (const uint64_t*)d_cnt,
                         (const uint64_t*)d_vscan, (const uint64_t*)d_bscan, w->bloom_k, (uint32_t)w->bloom_words, d_bits);
      WR_TRY(hipGetLastError());
    } else {
      WR_TRY(hipMemsetAsync(d_bits, 0, bloom_col, ctx->stream));
      WR_TRY(launch(bloom_global_kernel, G, true, 256, ctx->stream, cc, (uint32_t)ci, G, (const uint64_t*)d_cnt, (const uint64_t*)d_vscan,
                    (const uint64_t*)d_bscan, w->bloom_k, w->bloom_words, d_bits));
    }
  }
  return ORCGPU_OK;
}

// every stream of every column, enqueued from its description without a host wait, each into a slot of its bound.  Per column:
// the value streams, then PRESENT -- whose stream index is reserved first: the positions list it first
int wr_flush_streams(orcgpu_writer* w, WrFlush& F) {
  orcgpu_ctx* ctx = w->ctx;
  const uint64_t G = F.G, NJ = F.NJ;
  uint8_t* x = w->ix.p;
  for (size_t ci = 0; ci < w->cols.size(); ci++) {
    const WrCol& c = w->cols[ci];
    const WrColDev& d = w->dev[ci];
    WrStream sd[WR_MAX_STREAMS];
    const int ns = wr_streams(c, wr_counts(c), NJ != 0, sd);
    if (c.present && NJ) F.ix_streams[ci].push_back({F.streams.size() + (uint64_t)ns - 1, sd[ns - 1].pos_form});
    uint64_t unlisted = 0;  // streams just enqueued that the row index holds nothing for: their positions are zeroed
    for (int k = 0; k < ns; k++) {
      const WrStream& s = sd[k];
      const uint64_t li = F.streams.size();
      const bool is_present = s.src == WR_SRC_PRES;
      F.streams.push_back(WrStreamOut{s.stream, (uint32_t)ci + 1, F.at});
      WrIxPos ip{s.pos_mode, 0, 0, 0, nullptr, nullptr, 0, nullptr};
      if (s.pos_mode != WR_NO_POS) {
        if (!is_present) F.ix_streams[ci].push_back({li, s.pos_form});
        ip = WrIxPos{s.pos_mode, G, F.S, s.n, (const uint64_t*)(x + F.o_vscan) + ci * G, is_present ? nullptr : (const uint64_t*)(x + F.o_bscan) + ci * G,
                     is_present ? 0 : c.elem, (uint64_t*)(x + F.o_pos) + li * G * 4};
      }
      const WrIxPos* pip = is_present && !NJ ? nullptr : &ip;
      int rc = ORCGPU_OK;
      switch (s.enc) {
        case WR_ENC_RLE2: case WR_ENC_BYTE_RLE: rc = wr_rle_stream(w, s.enc, d.src(s.src), s.n, s.width, s.is_signed, &F.at, li, pip); break;
        case WR_ENC_BITS: rc = wr_bool_stream(w, d.src(s.src), s.n, &F.at, li, pip); break;
        case WR_ENC_COPY:
          rc = wr_copy_stream(w, d.src(s.src), s.n, &F.at, li, F.known);
          if (!rc && wr_ix_pos(ctx, &ip, nullptr) != hipSuccess) rc = ORCGPU_HIP_ERROR;
          break;
      }
      if (rc) return rc;
      unlisted = NJ && s.pos_mode == WR_NO_POS ? unlisted + 1 : 0;
      if (unlisted && (k + 1 == ns || sd[k + 1].pos_mode != WR_NO_POS))
        WR_TRY(hipMemsetAsync(w->ix.p + F.o_pos + (li + 1 - unlisted) * G * 32, 0, unlisted * G * 32, ctx->stream));
    }
  }
  return ORCGPU_OK;
}

// compression: every stream from its slot into its slot of zout, in one launch set; the lengths in w->lens become the chunks'
int wr_flush_compress(orcgpu_writer* w, WrFlush& F) {
  orcgpu_ctx* ctx = w->ctx;
  const uint64_t n_streams = F.n_streams;
  std::vector<LzcStream> jobs(n_streams);
  std::vector<uint64_t> rooms(n_streams);
  uint64_t zat = 0;
  for (uint64_t i = 0; i < n_streams; i++) {
    rooms[i] = (i + 1 < n_streams ? F.streams[i + 1].slot : F.at) - F.streams[i].slot;
    F.zslot[i] = zat;
    jobs[i] = LzcStream{F.streams[i].slot, zat, F.known[i]};
    zat += align_up(lzc_room(rooms[i], w->comp_block));
  }
  if (!wr_reserve(w, w->zout, zat + kAlign, 0)) {
    set_err(ctx, "writer: out of device memory (%llu bytes of compressed stripe)", (unsigned long long)zat);
    return ORCGPU_HIP_ERROR;
  }
  const LzcPlan* d_plan = nullptr;
  const uint64_t* d_chunk_off = nullptr;
  int rc = lzc_enqueue(ctx, lzc_codec(w->comp), w->comp_block, w->slots.p, w->zout.p, jobs, rooms, (uint64_t*)w->lens.p, &w->round_trips, &d_plan, &d_chunk_off);
  if (rc) return rc;
  if (F.NJ)
    WR_TRY(launch(ix_map_kernel, n_streams * F.G, false, 256, ctx->stream, n_streams * F.G, F.G, w->comp_block, d_plan, d_chunk_off, (uint64_t*)(w->ix.p + F.o_pos)));
  return ORCGPU_OK;
}

// the streams back to back on the device in the stripe's stream order, then one copy to pinned memory, and the wait for it
int wr_flush_pack(orcgpu_writer* w, WrFlush& F) {
  orcgpu_ctx* ctx = w->ctx;
  for (uint64_t i = 0; i < F.n_streams; i++) {
    if (F.known[i] != ~0ull && !F.comp) F.lens[i] = F.known[i];
    F.total += F.lens[i];
  }
  const uint64_t total = F.total;
  if (!wr_reserve(w, w->out, total + kAlign, 0)) return ORCGPU_HIP_ERROR;
  uint64_t pos = 0;
  for (uint64_t i = 0; i < F.n_streams; i++) {
    const uint8_t* src = F.comp ? w->zout.p + F.zslot[i] : w->slots.p + F.streams[i].slot;
    if (F.lens[i]) WR_TRY(hipMemcpyAsync(w->out.p + pos, src, F.lens[i], hipMemcpyDeviceToDevice, ctx->stream));
    pos += F.lens[i];
  }
  int rc = wr_pinned(w, w->pinned, w->pinned_cap, total, true);
  if (rc) return rc;
  if (total) WR_TRY(hipMemcpyAsync(w->pinned, w->out.p, total, hipMemcpyDeviceToHost, ctx->stream));
  return wr_sync(w);
}

// the stripe into the sink: the index streams (per column ROW_INDEX, then its BLOOM_FILTER_UTF8), data, footer; the writer's
// stripe state starts over
int wr_flush_finish(orcgpu_writer* w, WrFlush& F) {
  const std::vector<uint8_t> footer = wr_stripe_footer(w->cols, F.index, F.streams, F.lens, F.comp, w->comp_block, F.bloom);
  const uint64_t start = w->written;
  uint64_t index_length = 0;
  for (size_t ci = 0; ci < F.index.size(); ci++) {
    index_length += F.index[ci].size();
    int rc = wr_sink(w, F.index[ci].data(), F.index[ci].size());
    if (rc) return rc;
    if (!ci || !w->cols[ci - 1].bloom) continue;
    index_length += F.bloom[ci].size();
    rc = wr_sink(w, F.bloom[ci].data(), F.bloom[ci].size());
    if (rc) return rc;
  }
  int rc = wr_sink(w, w->pinned, F.total);
  if (rc) return rc;
  rc = wr_sink(w, footer.data(), footer.size());
  if (rc) return rc;
  w->stripes.push_back(WrStripe{start, F.total, footer.size(), w->rows, index_length});
  w->rows = 0;
  w->base_rle = 0;
  for (auto& c : w->cols) {
    if (c.is_utf8()) (c.dict ? w->n_dictionary : w->n_direct)++;
    c.dict = false;
    c.rows = c.n_valid = c.n_bytes = c.base_valid = 0;
  }
  return ORCGPU_OK;
}

// StripeWriter::finish_stripe (writer/stripe.rs:109-165) + ArrowWriter::flush_stripe.  Every stream of every column is enqueued
// without a host wait, each into a slot of its bound; then two waits, whatever the column count: the streams' lengths come back,
// and the streams, moved back to back on the device, reach the host in one copy.
int wr_flush(orcgpu_writer* w) {
  orcgpu_ctx* ctx = w->ctx;
  const uint64_t trips0 = w->round_trips;
  int rc = wr_dictionaries(w);
  if (rc) return rc;
  WrFlush F;
  rc = wr_flush_room(w, F);
  if (rc) return rc;
  const size_t nc = w->cols.size();
  F.comp = w->comp != ORCGPU_COMP_NONE;
  F.S = w->stride;
  F.G = w->stride ? (w->rows + F.S - 1) / F.S : 0;
  F.NJ = nc * F.G;
  F.ix_streams.resize(nc);
  if (F.NJ) rc = wr_flush_stats(w, F);
  if (!rc) rc = wr_flush_streams(w, F);
  F.zslot.assign(F.n_streams, 0);
  if (!rc && F.comp && F.n_streams) rc = wr_flush_compress(w, F);
  if (rc) return rc;
  // the row index comes back with the lengths
  if (F.NJ) WR_TRY(hipMemcpyAsync(w->ix_pinned, w->ix.p + F.o_recs, F.ix_span, hipMemcpyDeviceToHost, ctx->stream));
  F.lens.assign(F.n_streams, 0);
  if (F.n_streams) WR_TRY(hipMemcpyAsync(F.lens.data(), w->lens.p, F.n_streams * 8, hipMemcpyDeviceToHost, ctx->stream));
  rc = wr_sync(w);
  if (rc) return rc;
  if (w->stride) {  // ROW_INDEX streams (column 0 first) and the stripe's statistics
    std::vector<WrStat> stripe;
    F.index = wr_row_index(w->cols, w->rows, F.S, F.G, (const IxRec*)w->ix_pinned, (const uint64_t*)(w->ix_pinned + (F.o_pos - F.o_recs)),
                           w->ix_pinned + (F.o_side - F.o_recs), F.ix_streams, F.comp, w->comp_block, stripe);
    w->stripe_stats.push_back(std::move(stripe));
    // BLOOM_FILTER_UTF8 streams: the bitsets came back in the same copy; the framing around them is the host's
    F.bloom.resize(nc + 1);
    uint64_t nb = 0;
    for (size_t ci = 0; ci < nc; ci++)
      if (w->cols[ci].bloom)
        F.bloom[ci + 1] = wr_bloom_stream(w->bloom_k, w->bloom_words, F.G, w->ix_pinned + (F.o_bloom - F.o_recs) + nb++ * F.G * w->bloom_words * 8, F.comp,
                                          w->comp_block);
  }
  rc = wr_flush_pack(w, F);
  if (!rc) rc = wr_flush_finish(w, F);
  if (rc) return rc;
  w->stripe_round_trips += w->round_trips - trips0;
  return ORCGPU_OK;
}

}  // namespace
