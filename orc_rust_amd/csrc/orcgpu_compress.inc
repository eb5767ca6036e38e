// orcgpu_compress.inc -- host side of the stream compressor (device/lz_compress.hip): the launches of one call over any number of
// streams, used by the writer for a stripe's streams and by orcgpu_compress_stream for one.
namespace {

constexpr uint64_t kLzcDefaultBlock = 262144;          // compression.rs:31
constexpr uint64_t kLzcMaxBlock = (1ull << 23) - 1;    // a chunk header holds len * 2 + 1 in 24 bits

// the codec of the kernels (0 Snappy, 1 LZ4), or -1
inline int lzc_codec(int kind) { return kind == ORCGPU_COMP_SNAPPY ? 0 : (kind == ORCGPU_COMP_LZ4 ? 1 : -1); }
inline uint32_t lzc_seg_bytes(uint64_t B) { return (uint32_t)std::min<uint64_t>(LZC_SEG, B); }
inline uint64_t lzc_stride(uint32_t S) { return align_up(S + S / 8 + 64, 16); }  // a segment's body: its bytes and the elements' headers
// the room of a compressed stream of at most `raw` bytes: its bytes and 3 per chunk (a chunk never expands past its input)
inline uint64_t lzc_room(uint64_t raw, uint64_t B) { return raw + 3 * ((raw + B - 1) / B); }

#define LZC_TRY(expr)                                                                                     \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess) {                                                                               \
      set_err(ctx, "compress: %s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return ORCGPU_HIP_ERROR;                                                                            \
    }                                                                                                     \
  } while (0)

// Compresses streams i = 0 .. n-1: the raw bytes at d_in + jobs[i].in_off (at most rooms[i] of them), the chunks to
// d_out + jobs[i].out_off (room: lzc_room(rooms[i], B)).  Their lengths are jobs[i].known, or d_lens[i] on the device when the
// launches run; after them d_lens[i] holds the compressed lengths.  Enqueued on ctx->stream without a host wait (growing the
// tables waits: counted in *syncs).  d_plan / d_chunk_off (optional): where the chunk table is left (the streams' first chunks,
// n + 1 of them, and the compressed chunks' offsets): valid until the next call.
int lzc_enqueue(orcgpu_ctx* ctx, int codec, uint64_t B, const uint8_t* d_in, uint8_t* d_out, const std::vector<LzcStream>& jobs,
                const std::vector<uint64_t>& rooms, uint64_t* d_lens, uint64_t* syncs, const LzcPlan** d_plan_out = nullptr,
                const uint64_t** d_chunk_off_out = nullptr) {
  const uint32_t n = (uint32_t)jobs.size();
  if (!n) return ORCGPU_OK;
  hipStream_t st = ctx->stream;
  const uint32_t S = lzc_seg_bytes(B);
  const uint64_t stride = lzc_stride(S);
  uint64_t max_chunks = 0, max_segs = 0;
  for (uint64_t r : rooms) {
    const uint64_t c = (r + B - 1) / B;
    max_chunks += c;
    max_segs += (r + S - 1) / S + c;
  }
  if (max_segs >= 0xffffffffull || max_chunks + 1 >= 0xffffffffull) {
    set_err(ctx, "compress: %llu segments in one call", (unsigned long long)max_segs);
    return ORCGPU_INVALID_ARGUMENT;
  }
  const uint64_t n_size = max_chunks + 1;  // (the scan's last entry: the total)
  Bump T;
  const uint64_t o_jobs = T.take(n * sizeof(LzcStream)), o_plan = T.take((n + 1) * sizeof(LzcPlan)), o_meta = T.take(max_segs * sizeof(LzcSeg));
  const uint64_t o_size = T.take(n_size * 4), o_off = T.take(n_size * 8), o_sums = T.take((n_size / 2048 + 2) * 8), o_tot = T.take(16);
  if (syncs && (T.off + kAlign > ctx->lzc_tab.cap || max_segs * stride + kAlign > ctx->lzc_stage.cap)) ++*syncs;
  if (!ctx->lzc_tab.ensure(T.off + kAlign) || !ctx->lzc_stage.ensure(max_segs * stride + kAlign)) {
    set_err(ctx, "compress: out of device memory (%llu bytes of tables, %llu of segments)", (unsigned long long)T.off,
            (unsigned long long)(max_segs * stride));
    return ORCGPU_HIP_ERROR;
  }
  uint8_t* t = ctx->lzc_tab.p;
  LzcStream* d_jobs = (LzcStream*)(t + o_jobs);
  LzcPlan* d_plan = (LzcPlan*)(t + o_plan);
  LzcSeg* d_meta = (LzcSeg*)(t + o_meta);
  uint32_t* d_size = (uint32_t*)(t + o_size);
  uint64_t* d_off = (uint64_t*)(t + o_off);
  for (uint32_t i0 = 0; i0 < n; i0 += LZC_JOBS_PER_ARG) {
    LzcJobArgs a{};
    a.at = i0;
    a.n = std::min<uint32_t>(LZC_JOBS_PER_ARG, n - i0);
    for (uint32_t i = 0; i < a.n; i++) a.s[i] = jobs[i0 + i];
    LZC_TRY(launch(lzc_put_jobs_kernel, (uint64_t)1, true, 64, st, a, d_jobs));
  }
  LZC_TRY(launch(lzc_plan_kernel, (uint64_t)1, true, 1024, st, (const LzcStream*)d_jobs, n, d_lens, B, S, d_plan));
  LZC_TRY(launch(lzc_segment_kernel, max_segs, true, 64, st, codec, d_in, (const LzcStream*)d_jobs, (const LzcPlan*)d_plan, n, B, S, stride, d_meta,
                 ctx->lzc_stage.p));
  LZC_TRY(launch(lzc_chunk_size_kernel, n_size, true, 64, st, codec, (const LzcPlan*)d_plan, n, B, S, (const LzcSeg*)d_meta, d_size));
  int rc = enc_scan(ctx, st, (const uint32_t*)d_size, n_size, (uint64_t*)(t + o_sums), (uint64_t*)(t + o_tot), d_off);
  if (rc) return rc;
  LZC_TRY(launch(lzc_compose_kernel, max_chunks, true, 256, st, codec, d_in, (const LzcStream*)d_jobs, (const LzcPlan*)d_plan, n, B, S, stride,
                 (const LzcSeg*)d_meta, (const uint8_t*)ctx->lzc_stage.p, (const uint64_t*)d_off, d_out, d_lens));
  if (d_plan_out) *d_plan_out = d_plan;
  if (d_chunk_off_out) *d_chunk_off_out = d_off;
  return ORCGPU_OK;
}

}  // namespace

extern "C" int orcgpu_compress_stream(orcgpu_ctx* ctx, int kind, uint64_t block_size, const void* in, uint64_t n, uint32_t flags, uint8_t* out, uint64_t out_cap,
                                      uint64_t* out_len) {
  if (!ctx || !out_len || (n && !in)) return ORCGPU_INVALID_ARGUMENT;
  *out_len = 0;
  const int codec = lzc_codec(kind);
  if (kind == ORCGPU_COMP_ZLIB || kind == ORCGPU_COMP_LZO || kind == ORCGPU_COMP_ZSTD) {
    set_err(ctx, "compress: only Snappy and LZ4 streams are written");
    return ORCGPU_UNSUPPORTED;
  }
  const uint64_t B = block_size ? block_size : kLzcDefaultBlock;
  if (codec < 0 || B > kLzcMaxBlock) return ORCGPU_INVALID_ARGUMENT;
  const uint64_t bound = lzc_room(n, B);
  if (!out) {
    *out_len = bound;
    return ORCGPU_OK;
  }
  if (!n) return ORCGPU_OK;
  if (out_cap < bound) {
    set_err(ctx, "compress: the buffer holds %llu bytes, the bound is %llu", (unsigned long long)out_cap, (unsigned long long)bound);
    *out_len = bound;
    return ORCGPU_INVALID_ARGUMENT;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const bool on_device = flags & ORCGPU_ENC_ON_DEVICE;
  Bump I;
  const uint64_t o_in = I.take(on_device ? 0 : n), o_out = I.take(on_device ? 0 : bound), o_len = I.take(8);
  if (!ctx->lzc_io.ensure(I.off + kAlign)) {
    set_err(ctx, "compress: out of device memory (%llu bytes)", (unsigned long long)I.off);
    return ORCGPU_HIP_ERROR;
  }
  uint8_t* io = ctx->lzc_io.p;
  const uint8_t* d_in = (const uint8_t*)in;
  uint8_t* d_out = out;
  if (!on_device) {
    LZC_TRY(hipMemcpyAsync(io + o_in, in, n, hipMemcpyHostToDevice, st));
    d_in = io + o_in;
    d_out = io + o_out;
  }
  uint64_t* d_len = (uint64_t*)(io + o_len);
  int rc = lzc_enqueue(ctx, codec, B, d_in, d_out, {LzcStream{0, 0, n}}, {n}, d_len, nullptr);
  if (rc) return rc;
  uint64_t len = 0;
  LZC_TRY(hipMemcpyAsync(&len, d_len, 8, hipMemcpyDeviceToHost, st));
  LZC_TRY(hipStreamSynchronize(st));
  if (len > bound) {
    set_err(ctx, "compress: %llu bytes past the bound %llu", (unsigned long long)len, (unsigned long long)bound);
    return ORCGPU_UNEXPECTED;
  }
  if (!on_device) {
    LZC_TRY(hipMemcpyAsync(out, d_out, len, hipMemcpyDeviceToHost, st));
    LZC_TRY(hipStreamSynchronize(st));
  }
  *out_len = len;
  return ORCGPU_OK;
}
