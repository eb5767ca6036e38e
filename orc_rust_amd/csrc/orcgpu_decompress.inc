// orcgpu_decompress.inc -- chunk tables and launches of the block decompressors.
namespace {

inline double host_us_now() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct DecompPlan {
  uint64_t table_bytes = 0;      // host/pinned bytes of the tables
  uint64_t chunks_off = 0, streams_off = 0, zblocks_off = 0, zitems_off = 0;  // offsets inside the table blob
  uint64_t dev_off = 0;          // where the blob lives in scratch
  uint32_t n_chunks = 0, n_streams = 0, n_zblocks = 0, n_zitems = 0;
  uint64_t zdump_off = 0;        // sink for the idle lanes of zstd_entropy_kernel
  uint64_t zstatus_off = 0;      // two status words per ZBlock (sequences job, literals job), written by zstd_entropy_kernel
  uint64_t zprogress_off = 0;    // per ZBlock: sequences in memory so far (read by lz_exec_kernel while the entropy kernel runs); + the chunk queue's head
  uint64_t order_off = 0;        // inside the table blob: chunk indices in the order lz_exec_kernel takes them
  bool z_split_literals = false; // the literals are decoded by zstd_literals_kernel, in front of zstd_entropy_kernel
  bool z_lanes = false;          // the sequences go one lane per block (zstd_lanes.h): tables by zstd_entropy_kernel, then zstd_seq_lanes_kernel
  uint64_t z_total_seq = 0;
  uint32_t n_zchains = 0;        // blocks that have sequences: ZBlocks [0, n_zchains) (most sequences first)
  uint64_t ztab_off = 0, zhdr_off = 0;  // z_lanes: 2560 bytes of table cells + a ZSeqHdr per chain
  uint64_t chunk_start_off = 0;  // per chunk: where its plain bytes start in its stream (written by the finalize kernel)
  TableCounts counts;                    // the streams' tables added up, their orders merged (orcgpu_decomp_plan.inc)
  std::vector<uint64_t> stream_scratch;  // per stream: scratch offset of its record / literal / sequence scratch, ~0 if it needs none
};

// The streams' tables were built when they were staged (StagedStream::tables): a call adds up their counts, merges their block
// orders and hands out the bases; launch_decompress copies and rebases the entries.
int plan_decompress(Plan& P, DecompPlan& DP) {
  if (P.decomp.empty()) return ORCGPU_OK;
  const size_t ns = P.decomp.size();
  {
    std::vector<const StreamTables*> t(ns);
    for (size_t k = 0; k < ns; k++) t[k] = &P.decomp[k].st->tables;
    tables_count(t.data(), ns, DP.counts);
  }
  const TableCounts& C = DP.counts;
  DP.n_streams = C.n_streams;
  DP.n_chunks = C.n_chunks;
  DP.n_zblocks = C.n_zblocks;
  DP.n_zitems = C.n_zitems;
  DP.n_zchains = C.n_zchains;
  DP.z_total_seq = C.total_seq;
  {
    // Entropy jobs are taken in index order: the blocks with the most sequences (the longest serial chains) get the lowest
    // indices, so they start when the kernel does and the short ones fill in around them (the streams carry their blocks in that
    // order: the call's order is their merge, TableCounts::zb_at).
    // One lane per block instead of one wavefront (zstd_lanes.h) when the call is a throughput matter: the wavefront-per-block
    // stage takes about 0.1 ns of the whole chip per sequence, a chain on its own lane about 200 ns per sequence whatever
    // runs beside it.  ORCGPU_ZSTD_LANES=0 / 1 forces either (tests run both).
    const char* force = getenv("ORCGPU_ZSTD_LANES");  // (read per call: the tests switch it between calls)
    const uint64_t min_seq = kZstdLanesMinSequences;
    DP.z_lanes = DP.n_zchains && (force ? atoi(force) != 0 : (P.call_z_lanes >= 0 ? P.call_z_lanes != 0 : C.total_seq >= min_seq));
    // the literals as a kernel of their own (a third of the LDS: three times the wavefronts) in that mode.  Not with one wavefront
    // per block: the execution kernel then runs BESIDE the entropy kernel and needs a block's literals first -- behind a literals
    // kernel that fills the machine its workgroups only wait (SF 12.5: 90 -> 135 ms).
    DP.z_split_literals = DP.z_lanes;
  }
  // every stream's record, literal and sequence scratch, laid out when it was staged: 8 bytes per sequence when they go one lane per
  // block (packed records), 12 when one wavefront decodes a block (three arrays)
  DP.stream_scratch.assign(ns, ~0ull);
  const uint32_t seq_bytes = DP.z_lanes ? kSeqBytesPacked : kSeqBytesArrays;
  for (size_t k = 0; k < ns; k++) {
    const uint64_t need = P.decomp[k].st->tables.scratch_bytes(seq_bytes);
    if (need) DP.stream_scratch[k] = P.scratch.take(need, 16);
  }
  if (DP.z_lanes) {
    DP.ztab_off = P.scratch.take((uint64_t)DP.n_zchains * ZL_CELLS * 2 + 16, 16);
    DP.zhdr_off = P.scratch.take((uint64_t)DP.n_zchains * sizeof(ZSeqHdr) + 16, 16);
  }
  if (DP.n_zblocks) DP.zdump_off = P.scratch.take(1024 * 64 * 4);
  DP.zstatus_off = P.scratch.take(8ull * DP.n_zblocks + 16);  // two jobs per block
  DP.zprogress_off = P.scratch.take(4ull * DP.n_zblocks + 16);  // [n_zblocks] = the queue head
  DP.chunk_start_off = P.scratch.take(4ull * DP.n_chunks + 16);
  Bump b;
  DP.chunks_off = b.take((uint64_t)DP.n_chunks * sizeof(ChunkDesc), 16);
  DP.streams_off = b.take((uint64_t)DP.n_streams * sizeof(StreamDesc), 16);
  DP.zblocks_off = b.take((uint64_t)DP.n_zblocks * sizeof(ZBlock), 16);
  DP.zitems_off = b.take((uint64_t)DP.n_zitems * sizeof(ZItem), 16);
  DP.order_off = b.take((uint64_t)DP.n_chunks * 4, 16);
  DP.table_bytes = align_up(b.off, 16);
  DP.dev_off = P.scratch.take(DP.table_bytes);
  return ORCGPU_OK;
}

// Zstandard's two stages side by side (see launch_chunk_decoders)?  Not when the call also has DEFLATE chunks: the execution
// kernel takes their tokens from inflate_parse_kernel, behind it.
static bool decomp_side_by_side(const orcgpu_ctx* ctx, const ChunkDesc* h_chunks, uint32_t n_chunks, uint32_t n_zblocks, bool z_lanes) {
  if (z_lanes) return false;  // (one lane per block: the execution kernel runs behind the sequences kernel)
  constexpr bool use_inflate_parse = true;
  bool deflate = false;
  for (uint32_t i = 0; i < n_chunks; i++) deflate = deflate || h_chunks[i].kind == 1;
  return n_zblocks && ctx->aux_stream && !(deflate && use_inflate_parse);
}

// host_blob: pinned memory behind the summary mirror
// One launch per codec family present in the chunk table (plain "original" chunks ride with the first).
static int launch_chunk_decoders(orcgpu_ctx* ctx, hipStream_t st, ChunkDesc* d_chunks, const ChunkDesc* h_chunks, uint32_t n_chunks, ZBlock* d_zblocks,
                                 uint32_t n_zblocks, const ZItem* d_zitems, uint32_t* d_zdump, uint32_t* d_zstatus, uint32_t* d_zprogress, const uint32_t* d_order, hipEvent_t stage1_done = nullptr,
                                 uint32_t n_zchains = 0, uint16_t* d_ztab = nullptr, ZSeqHdr* d_zhdr = nullptr, bool split_literals = false, hipEvent_t tables_ev = nullptr,
                                 hipEvent_t seq_done_ev = nullptr) {
  bool deflate = false, tokens = false, others = false, lzo = false;
  // DEFLATE: tokens by inflate_parse_kernel (64 lanes per chunk), copies by lz_exec_kernel; what they leave alone, and everything
  // when ORCGPU_NO_INFLATE_PARSE is set, goes to the one-wavefront decoder
  constexpr bool use_inflate_parse = true;
  for (uint32_t i = 0; i < n_chunks; i++) {
    const uint32_t k = h_chunks[i].kind;
    if (k == 1) deflate = true;
    else if (k == 3) lzo = true;
    else others = true;  // Zstandard, Snappy, LZ4, copies and anything unknown (flagged by the kernel)
    if (k == 2 || k == 4) tokens = true;
  }
  if (deflate && use_inflate_parse) others = true;
  int copy_too = 1;
  if (others) {
    // entropy stage (Zstandard: one wavefront per job) / token stage (Snappy, LZ4: one workgroup per chunk), then LZ77 execution
    // (one workgroup per chunk).  Zstandard's two stages run SIDE BY SIDE: the execution kernel goes to a second stream and takes
    // every block's sequences as the entropy kernel publishes them (a block's FSE chain is serial: the longest block would
    // otherwise be decoded first and executed afterwards, one after the other).
    // (not when the call also has DEFLATE chunks: the execution kernel takes their tokens from inflate_parse_kernel, behind it)
    const bool side = decomp_side_by_side(ctx, h_chunks, n_chunks, n_zblocks, d_ztab != nullptr);
    if (n_zblocks) HIP_TRY(ctx, hipMemsetAsync(d_zstatus, 0xff, 8ull * n_zblocks, st));  // ZSTD_PENDING
    HIP_TRY(ctx, hipMemsetAsync(d_zprogress, 0, 4ull * n_zblocks + 8, st));             // (+ the queue head, + the count of entropy jobs that have ended)
    if (side) {
      HIP_TRY(ctx, hipEventRecord(ctx->aux_ev[0], st));
      HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux_stream, ctx->aux_ev[0], 0));
    }
    // (one lane per block: the literals are a kernel of their own -- a third of the LDS, three times the wavefronts --, the entropy
    // kernel only builds the FSE tables: jobs [0, n_zblocks))
    // The sequences kernel (one lane per block) lasts as long as the longest chains and needs only the FSE tables: the literals are
    // decoded beside it, on the second stream (ORCGPU_ZSTD_LIT_ASIDE=0: in front of it, on this one)
    const bool lit_aside = split_literals && d_ztab && ctx->aux_stream && !(getenv("ORCGPU_ZSTD_LIT_ASIDE") && atoi(getenv("ORCGPU_ZSTD_LIT_ASIDE")) == 0);
    if (n_zblocks && split_literals && !lit_aside)
      HIP_TRY(ctx, launch(zstd_literals_kernel, (uint64_t)n_zblocks, true, 64, st, (const ZBlock*)d_zblocks, n_zblocks, d_zstatus, d_zprogress));
    if (n_zblocks) HIP_TRY(ctx, launch(zstd_entropy_kernel, (split_literals ? 1ull : 2ull) * n_zblocks, true, 64, st, (const ZBlock*)d_zblocks, n_zblocks, d_zdump, d_zstatus, d_zprogress, d_ztab, d_zhdr));
    if (d_ztab && n_zchains) {
      if (tables_ev) HIP_TRY(ctx, hipEventRecord(tables_ev, st));
      if (tables_ev) ctx->tables_gate.store(1, std::memory_order_release);
      // (the other lanes' table kernels first -- in front of this lane's sequences kernel AND its literals kernel, which fills what
      // LDS the sequences kernel leaves: see orcgpu_ctx::tables_gate.  Their host threads run beside this one: wait -- bounded --
      // until each has enqueued its kernel, then let the stream wait for it)
      const double t_gate = host_us_now();
      for (int k = 0; k < ctx->n_gate_peers; k++) {
        orcgpu_ctx* peer = ctx->gate_peers[k];
        int g = 0;
        for (int spins = 0; spins < 100000 && !(g = peer->tables_gate.load(std::memory_order_acquire)); spins++) std::this_thread::yield();
        if (g == 1) HIP_TRY(ctx, hipStreamWaitEvent(st, peer->ev[7], 0));
      }
      ctx->hp_gate += host_us_now() - t_gate;
      if (tables_ev) HIP_TRY(ctx, hipEventRecord(ctx->ev[9], st));  // (the sequences kernel's span starts here: behind the waits)
    }
    if (n_zblocks && lit_aside) HIP_TRY(ctx, hipEventRecord(ctx->aux_ev[0], st));  // (the status words are set, the tables built)
    if (d_ztab && n_zchains) {
      // 16 chains per wavefront, four lanes each: four wavefronts per CU, one per SIMD, all of its LDS
      HIP_TRY(ctx, launch(zstd_seq_quads_kernel, (uint64_t)(n_zchains + 15) / 16, true, 64, st, (const ZBlock*)d_zblocks, n_zchains, (const uint16_t*)d_ztab, (const ZSeqHdr*)d_zhdr, d_zstatus));
      if (seq_done_ev) HIP_TRY(ctx, hipEventRecord(seq_done_ev, st));  // (the sequences kernel alone: in front of the wait for the literals kernel beside it)
    }
    if (n_zblocks && lit_aside) {
      // (launched behind the sequences kernel: that one takes the LDS it needs first, the literals fill in around it)
      HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux_stream, ctx->aux_ev[0], 0));
      HIP_TRY(ctx, hipEventRecord(ctx->lit_ev[0], ctx->aux_stream));  // (the literals kernel's own span: orcgpu_last_lane_stats)
      HIP_TRY(ctx, launch(zstd_literals_kernel, (uint64_t)n_zblocks, true, 64, ctx->aux_stream, (const ZBlock*)d_zblocks, n_zblocks, d_zstatus, d_zprogress));
      HIP_TRY(ctx, hipEventRecord(ctx->lit_ev[1], ctx->aux_stream));
      ctx->lit_ev_used = true;
      HIP_TRY(ctx, hipEventRecord(ctx->aux_ev[1], ctx->aux_stream));
      HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->aux_ev[1], 0));
    }
    if (tokens) HIP_TRY(ctx, launch(lz_parse_kernel, (uint64_t)n_chunks, true, 64 * LZP_WAVES, st, d_chunks, n_chunks));
    if (deflate && use_inflate_parse) {
      // few chunks: four wavefronts per chunk (the call lasts as long as its longest chunk's chain of windows: C3 / zlib 11.6 -> 5.3 ms);
      // chunks enough to fill the device several times over: one (lineitem SF 4, 4.7 k chunks: four were 20 % slower)
      const bool four = n_chunks <= 6u * (ctx->n_cus ? ctx->n_cus : 256u);
      ctx->dbg_inflate_threads = four ? 256u : 64u;
      if (four) {
        HIP_TRY(ctx, launch(inflate_parse4_kernel, (uint64_t)n_chunks, true, 256, st, d_chunks, n_chunks, 0u, 0xffffffffu));
      } else {
        HIP_TRY(ctx, launch(inflate_parse_kernel, (uint64_t)n_chunks, true, 64, st, d_chunks, n_chunks, 0u, 0xffffffffu));
      }
    }
    if (stage1_done) HIP_TRY(ctx, hipEventRecord(stage1_done, st));
    stage1_done = nullptr;
    if (tokens) {
      const bool four = n_chunks > 4u * (ctx->n_cus ? ctx->n_cus : 256u);
      if (four) HIP_TRY(ctx, launch(lz_exec_tokens4_kernel, (uint64_t)n_chunks, true, 256, st, d_chunks, n_chunks));
      else HIP_TRY(ctx, launch(lz_exec_tokens_kernel, (uint64_t)n_chunks, true, LZT_THREADS, st, d_chunks, n_chunks));
    }
    hipStream_t xs = side ? ctx->aux_stream : st;
    // (a grid that is resident at once and leaves room: two workgroups per CU -- the kernel's registers allow four, but with
    // three resident everywhere the entropy kernel's workgroups were not placed any more: measured, MI355X.  Alone: four)
    // (ORCGPU_EXEC_PATIENCE: polls a workgroup waits for the entropy kernel; 0 = every chunk not ready at once is put off -- test hook)
    const char* pe = getenv("ORCGPU_EXEC_PATIENCE");
    const uint32_t patience = pe ? (uint32_t)atoll(pe) : (uint32_t)LZX_WATCHDOG;
    const uint64_t xgrid = std::min<uint64_t>(n_chunks, (side ? 512ull / LZX_THREADS : 1024ull / LZX_THREADS) * (ctx->n_cus ? ctx->n_cus : 256));
    // (one lane per block: one chunk per workgroup, no queue -- ORCGPU_EXEC_QUEUE=1 keeps the persistent grid --, and workgroups of
    // one wavefront -- ORCGPU_EXEC_WAVE=0 keeps four)
    // (... and whenever the execution kernel has nothing to wait for and thousands of chunks to go through: a DEFLATE table)
    const bool single_shot = d_ztab != nullptr || (!side && n_chunks >= 2048);
    const bool wave_groups = single_shot;
    if (deflate) ctx->dbg_exec_threads = wave_groups ? 64u : (uint32_t)LZX_THREADS;
    if (wave_groups)
      HIP_TRY(ctx, launch(lz_exec_wave_kernel, (uint64_t)n_chunks, true, 64, xs, d_chunks, n_chunks, d_zitems, (const ZBlock*)d_zblocks, (const uint32_t*)d_zstatus,
                          (const uint32_t*)d_zprogress, n_zblocks, copy_too, d_order));
    else
    HIP_TRY(ctx, launch(lz_exec_kernel, single_shot ? (uint64_t)n_chunks : xgrid, true, LZX_THREADS, xs, d_chunks, n_chunks, d_zitems, (const ZBlock*)d_zblocks, (const uint32_t*)d_zstatus,
                        (const uint32_t*)d_zprogress, n_zblocks, copy_too, d_order, single_shot ? (uint32_t*)nullptr : d_zprogress + n_zblocks, side ? 0 : 2, patience));
    if (side) {
      HIP_TRY(ctx, hipEventRecord(ctx->aux_ev[1], ctx->aux_stream));
      HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->aux_ev[1], 0));
      // behind both kernels: the chunks the first launch did not get to before the entropy kernel ended (its grid had to leave
      // room for that kernel; this one fills the machine) and whatever it put off.  Such chunks still carry LZX_DEFERRED (set
      // by the host for this mode); the queue is gone through once more
      const uint64_t xgrid2 = std::min<uint64_t>(n_chunks, (1024ull / LZX_THREADS) * (ctx->n_cus ? ctx->n_cus : 256));
      HIP_TRY(ctx, hipMemsetAsync(d_zprogress + n_zblocks, 0, 4, st));
      HIP_TRY(ctx, launch(lz_exec_kernel, xgrid2, true, LZX_THREADS, st, d_chunks, n_chunks, d_zitems, (const ZBlock*)d_zblocks, (const uint32_t*)d_zstatus,
                          (const uint32_t*)d_zprogress, n_zblocks, copy_too, d_order, d_zprogress + n_zblocks, 1, (uint32_t)LZX_WATCHDOG));
    }
    copy_too = 0;
  }
  if (stage1_done) HIP_TRY(ctx, hipEventRecord(stage1_done, st));
  if (lzo) {
    // LZO1X: one wavefront per chunk (the "original" chunks of the stripe went with the execution kernel above)
    HIP_TRY(ctx, launch(decompress_lzo_kernel, (uint64_t)n_chunks, true, 64, st, d_chunks, n_chunks));
  }
  if (deflate) HIP_TRY(ctx, launch(decompress_deflate_kernel, (uint64_t)n_chunks, true, 64, st, d_chunks, n_chunks, copy_too, use_inflate_parse ? 1 : 0));
  return ORCGPU_OK;
}

int launch_decompress(orcgpu_ctx* ctx, Plan& P, DecompPlan& DP, uint8_t* S, uint64_t* d_scalars, uint8_t* host_blob, hipEvent_t stage1 = nullptr, hipEvent_t tables_ev = nullptr,
                      hipEvent_t done_ev = nullptr, hipEvent_t seq_done_ev = nullptr) {
  if (!(DP.z_lanes && DP.n_zchains && DP.n_chunks)) ctx->tables_gate.store(2, std::memory_order_release);  // (no table kernel in this lane's call: nobody waits for it)
  if (tables_ev && !(DP.z_lanes && DP.n_zchains && DP.n_chunks)) HIP_TRY(ctx, hipEventRecord(tables_ev, ctx->stream));  // (no such kernel in this call: an empty span)
  if (!DP.n_streams || !DP.n_chunks) {
    if (stage1) HIP_TRY(ctx, hipEventRecord(stage1, ctx->stream));
    if (!DP.n_streams) {
      if (done_ev) HIP_TRY(ctx, hipEventRecord(done_ev, ctx->stream));
      return ORCGPU_OK;
    }
    stage1 = nullptr;
  }
  hipStream_t st = ctx->stream;
  const double t_fill = host_us_now();
  ChunkDesc* hc = reinterpret_cast<ChunkDesc*>(host_blob + DP.chunks_off);
  StreamDesc* hstr = reinterpret_cast<StreamDesc*>(host_blob + DP.streams_off);
  ZBlock* hzb = reinterpret_cast<ZBlock*>(host_blob + DP.zblocks_off);
  ZItem* hzi = reinterpret_cast<ZItem*>(host_blob + DP.zitems_off);
  {
    // the streams' prebuilt entries, copied and rebased (tables_fill): their arenas, plain buffers and scratch, their places in the call
    std::vector<StreamUse> use(P.decomp.size());
    for (size_t si = 0; si < use.size(); si++) {
      const DecompStream& ds = P.decomp[si];
      StreamUse& u = use[si];
      u.t = &ds.st->tables;
      u.arena = ds.stripe->dev;
      u.plain = ds.result_index >= 0 ? P.results[ds.result_index]->arena[ctx->lane_id].p + ds.result_off : S + ds.scratch_off;
      u.scratch = DP.stream_scratch[si] != ~0ull ? S + DP.stream_scratch[si] : nullptr;
      u.len_idx = ds.len_idx;
      u.err_idx = ds.err_idx;
      u.framing_error = ds.st->framing_error ? 1 : 0;
      u.skip = ds.st->skip_bytes;
    }
    tables_fill(use.data(), DP.counts, DP.z_lanes, hc, hstr, hzb, hzi, reinterpret_cast<uint32_t*>(host_blob + DP.order_off));
  }
  if (decomp_side_by_side(ctx, hc, DP.n_chunks, DP.n_zblocks, DP.z_lanes))
    // the execution kernel runs twice in that mode, beside the entropy kernel and behind it: a chunk is the second launch's
    // as long as it carries this mark (the first launch replaces it with the chunk's outcome)
    for (uint32_t c = 0; c < DP.n_chunks; c++)
      if (hc[c].kind == 5 || hc[c].kind == 0) hc[c].diag = LZX_DEFERRED;
  ChunkDesc* d_chunks = reinterpret_cast<ChunkDesc*>(S + DP.dev_off + DP.chunks_off);
  StreamDesc* d_streams = reinterpret_cast<StreamDesc*>(S + DP.dev_off + DP.streams_off);
  ZBlock* d_zblocks = reinterpret_cast<ZBlock*>(S + DP.dev_off + DP.zblocks_off);
  ZItem* d_zitems = reinterpret_cast<ZItem*>(S + DP.dev_off + DP.zitems_off);
  const double t_up = host_us_now();
  ctx->hp_fill += t_up - t_fill;
  HIP_TRY(ctx, hipMemcpyAsync(S + DP.dev_off, host_blob, DP.table_bytes, hipMemcpyHostToDevice, st));
  ctx->hp_upload += host_us_now() - t_up;
  if (DP.n_chunks) {
    int rc = launch_chunk_decoders(ctx, st, d_chunks, hc, DP.n_chunks, d_zblocks, DP.n_zblocks, d_zitems, reinterpret_cast<uint32_t*>(S + DP.zdump_off),
                                   reinterpret_cast<uint32_t*>(S + DP.zstatus_off), reinterpret_cast<uint32_t*>(S + DP.zprogress_off), reinterpret_cast<const uint32_t*>(S + DP.dev_off + DP.order_off), stage1,
                                   DP.n_zchains, DP.z_lanes ? reinterpret_cast<uint16_t*>(S + DP.ztab_off) : nullptr, DP.z_lanes ? reinterpret_cast<ZSeqHdr*>(S + DP.zhdr_off) : nullptr, DP.z_split_literals, tables_ev, seq_done_ev);
    if (rc) return rc;
  }
  // (the block decoders end here: the kernel that strings the chunks' plain bytes together counts with the walk -- beside another
  // lane's execution kernel it waits for slots, 7 ms at table scale, and that wait is no decoder's time)
  if (done_ev) HIP_TRY(ctx, hipEventRecord(done_ev, st));
  HIP_TRY(ctx, launch(decompress_finalize_kernel, (uint64_t)DP.n_streams, true, 64, st, (const ChunkDesc*)d_chunks, (const StreamDesc*)d_streams, d_scalars,
                      reinterpret_cast<uint32_t*>(S + DP.chunk_start_off)));
  return ORCGPU_OK;
}

}  // namespace
