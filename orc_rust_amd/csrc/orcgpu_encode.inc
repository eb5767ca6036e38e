// orcgpu_encode.inc -- host side of the device encoders (device/rle_encode.hip): the launches of one stream's pipeline, and a
// column's streams as ColumnStripeEncoder::{encode_array, finish} hands them to the stripe writer (src/writer/column.rs).
namespace {

struct EncJob {          // one stream through the pipeline: planned (sizes known), then written
  int kind = 0;          // 0 Integer RLE v2, 1 byte RLE
  const void* values = nullptr;  // device
  uint64_t n = 0;
  int int_bytes = 8, is_signed = 1;
  uint32_t n_runs = 0, rpw = 64;
  uint64_t total = 0;
  // device tables (in ctx->enc_a / enc_b)
  uint16_t* next16 = nullptr;
  uint32_t* runs = nullptr;
  uint32_t* run_bytes = nullptr;
  EncRun* recs = nullptr;
  uint64_t* offsets = nullptr;
  // deferred (the stripe writer): no host waits -- tables sized for n runs, the run count and the size stay on the device
  bool deferred = false;
  const uint64_t* d_n_runs = nullptr;
  const uint64_t* d_total = nullptr;
  uint64_t* syncs = nullptr;  // counts the host waits of the plan (and the growth of its tables, which waits too)
};

#define ENC_TRY(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) {                                                                             \
      set_err(ctx, "encode: %s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return ORCGPU_HIP_ERROR;                                                                          \
    }                                                                                                   \
  } while (0)

// exclusive scan of `count` u32 into u64 (+ the total, left in *d_total); d_sums: (count + 2047) / 2048 words
int enc_scan(orcgpu_ctx* ctx, hipStream_t st, const uint32_t* d_in, uint64_t count, uint64_t* d_sums, uint64_t* d_total, uint64_t* d_out) {
  const uint32_t n_sums = (uint32_t)((count + 2047) / 2048);
  ENC_TRY(launch(enc_scan_tiles_kernel, (uint64_t)n_sums, true, 256, st, d_in, count, d_sums));
  ENC_TRY(launch(enc_scan_sums_kernel, (uint64_t)1, true, 1024, st, d_sums, n_sums, d_total));
  ENC_TRY(launch(enc_scan_apply_kernel, (uint64_t)n_sums, true, 256, st, d_in, count, (const uint64_t*)d_sums, d_out));
  return ORCGPU_OK;
}

// the runs of a stream and their sizes: J.total bytes when written
int enc_plan(orcgpu_ctx* ctx, EncJob& J) {
  hipStream_t st = ctx->stream;
  J.n_runs = 0;
  J.total = 0;
  if (!J.n) return ORCGPU_OK;
  if (J.n >= 0xffffffffull - 1024) {
    set_err(ctx, "encode: %llu values in one stream (fewer than 2^32 - 1024 per call)", (unsigned long long)J.n);
    return ORCGPU_INVALID_ARGUMENT;
  }
  // levels of exit maps: tiles of 512 positions, spans of 32 maps each level up, until 32 or fewer are left
  std::vector<uint32_t> cnt;
  cnt.push_back((uint32_t)((J.n + ENC_TILE - 1) / ENC_TILE));
  while (cnt.back() > ENC_FAN) cnt.push_back((cnt.back() + ENC_FAN - 1) / ENC_FAN);
  const size_t levels = cnt.size();
  Bump A;
  const uint64_t o_next = A.take((uint64_t)cnt[0] * ENC_TILE * 2);
  std::vector<uint64_t> o_map(levels), o_ent(levels);
  for (size_t l = 0; l < levels; l++) {
    o_map[l] = A.take((uint64_t)cnt[l] * ENC_TILE * 2);
    o_ent[l] = A.take((uint64_t)cnt[l] * 2);
  }
  const uint64_t o_tile_runs = A.take((uint64_t)cnt[0] * 4), o_tile_off = A.take((uint64_t)cnt[0] * 8);
  const uint64_t o_sums = A.take(((uint64_t)cnt[0] / 2048 + 2) * 8), o_total = A.take(16);
  if (J.syncs && A.off + kAlign > ctx->enc_a.cap) ++*J.syncs;
  if (!ctx->enc_a.ensure(A.off + kAlign)) {
    set_err(ctx, "encode: out of device memory (%llu bytes of chain tables)", (unsigned long long)A.off);
    return ORCGPU_HIP_ERROR;
  }
  uint8_t* a = ctx->enc_a.p;
  J.next16 = (uint16_t*)(a + o_next);
  auto map = [&](size_t l) { return (uint16_t*)(a + o_map[l]); };
  auto ent = [&](size_t l) { return (uint16_t*)(a + o_ent[l]); };
  uint32_t* d_tile_runs = (uint32_t*)(a + o_tile_runs);
  uint64_t* d_tile_off = (uint64_t*)(a + o_tile_off);
  uint64_t* d_sums = (uint64_t*)(a + o_sums);
  uint64_t* d_total = (uint64_t*)(a + o_total);
  if (J.kind == 0)
    ENC_TRY(launch(enc_next_kernel<0>, (uint64_t)cnt[0], true, 512, st, J.values, J.n, J.int_bytes, J.next16, map(0)));
  else
    ENC_TRY(launch(enc_next_kernel<1>, (uint64_t)cnt[0], true, 512, st, J.values, J.n, 1, J.next16, map(0)));
  for (size_t l = 0; l + 1 < levels; l++)
    ENC_TRY(launch(enc_compose_kernel, (uint64_t)cnt[l + 1], true, 512, st, (const uint16_t*)map(l), cnt[l], map(l + 1)));
  // back down: the top level's maps are entered from offset 0 of the first
  ENC_TRY(launch(enc_entries_kernel, (uint64_t)1, true, 64, st, (const uint16_t*)map(levels - 1), cnt[levels - 1], (const uint16_t*)nullptr, 1u, ent(levels - 1)));
  for (size_t l = levels - 1; l-- > 0;)
    ENC_TRY(launch(enc_entries_kernel, (uint64_t)(cnt[l + 1] + 63) / 64, true, 64, st, (const uint16_t*)map(l), cnt[l], (const uint16_t*)ent(l + 1), cnt[l + 1], ent(l)));
  const uint64_t tile_wgs = ((uint64_t)cnt[0] + 3) / 4;
  if (J.kind == 0)
    ENC_TRY(launch(enc_runs_kernel<0>, tile_wgs, true, 256, st, (const uint16_t*)J.next16, J.n, (const uint16_t*)ent(0), cnt[0], d_tile_runs, (const uint64_t*)nullptr,
                   (uint32_t*)nullptr, (uint32_t*)nullptr));
  else
    ENC_TRY(launch(enc_runs_kernel<1>, tile_wgs, true, 256, st, (const uint16_t*)J.next16, J.n, (const uint16_t*)ent(0), cnt[0], d_tile_runs, (const uint64_t*)nullptr,
                   (uint32_t*)nullptr, (uint32_t*)nullptr));
  int rc = enc_scan(ctx, st, d_tile_runs, cnt[0], d_sums, d_total, d_tile_off);
  if (rc) return rc;
  uint64_t n_runs = J.n;  // deferred: as many as there can be
  if (!J.deferred) {
    ENC_TRY(hipMemcpyAsync(&n_runs, d_total, 8, hipMemcpyDeviceToHost, st));
    ENC_TRY(hipStreamSynchronize(st));
    if (J.syncs) ++*J.syncs;
  }
  if (!n_runs || n_runs > J.n) {
    set_err(ctx, "encode: %llu runs for %llu values", (unsigned long long)n_runs, (unsigned long long)J.n);
    return ORCGPU_UNEXPECTED;
  }
  J.n_runs = (uint32_t)n_runs;
  Bump B;
  const uint64_t o_runs = B.take(n_runs * 4), o_bytes = B.take(n_runs * 4), o_recs = B.take(J.kind == 0 ? n_runs * sizeof(EncRun) : 8);
  const uint64_t o_offs = B.take(n_runs * 8), o_sums2 = B.take((n_runs / 2048 + 2) * 8), o_total2 = B.take(16);
  if (J.syncs && B.off + kAlign > ctx->enc_b.cap) ++*J.syncs;
  if (!ctx->enc_b.ensure(B.off + kAlign)) {
    set_err(ctx, "encode: out of device memory (%llu bytes of run tables)", (unsigned long long)B.off);
    return ORCGPU_HIP_ERROR;
  }
  uint8_t* b = ctx->enc_b.p;
  J.runs = (uint32_t*)(b + o_runs);
  J.run_bytes = (uint32_t*)(b + o_bytes);
  J.recs = (EncRun*)(b + o_recs);
  J.offsets = (uint64_t*)(b + o_offs);
  J.d_n_runs = J.deferred ? d_total : nullptr;
  if (J.deferred) ENC_TRY(hipMemsetAsync(J.run_bytes, 0, n_runs * 4, st));  // (the runs past the count add nothing to the scan)
  if (J.kind == 0) {
    ENC_TRY(launch(enc_runs_kernel<0>, tile_wgs, true, 256, st, (const uint16_t*)J.next16, J.n, (const uint16_t*)ent(0), cnt[0], d_tile_runs, (const uint64_t*)d_tile_off,
                   J.runs, J.run_bytes));
    // runs per wavefront: short runs are settled by a lane each (64 of them), long literals one after the other by the wavefront (4)
    J.rpw = J.deferred ? 64u : (J.n / n_runs >= 128 ? 4u : (J.n / n_runs >= 32 ? 16u : 64u));
    const uint64_t wgs = (n_runs + 4ull * J.rpw - 1) / (4ull * J.rpw);
    ENC_TRY(launch(enc2_plan_kernel, wgs, true, 256, st, J.values, J.int_bytes, J.is_signed, (const uint16_t*)J.next16, (const uint32_t*)J.runs, J.n_runs, J.recs,
                   J.run_bytes, J.rpw, J.d_n_runs));
  } else {
    ENC_TRY(launch(enc_runs_kernel<1>, tile_wgs, true, 256, st, (const uint16_t*)J.next16, J.n, (const uint16_t*)ent(0), cnt[0], d_tile_runs, (const uint64_t*)d_tile_off,
                   J.runs, J.run_bytes));
  }
  rc = enc_scan(ctx, st, J.run_bytes, n_runs, (uint64_t*)(b + o_sums2), (uint64_t*)(b + o_total2), J.offsets);
  if (rc) return rc;
  J.d_total = (const uint64_t*)(b + o_total2);
  if (J.deferred) return ORCGPU_OK;  // (J.total unknown: the caller's room is its bound)
  ENC_TRY(hipMemcpyAsync(&J.total, b + o_total2, 8, hipMemcpyDeviceToHost, st));
  ENC_TRY(hipStreamSynchronize(st));
  if (J.syncs) ++*J.syncs;
  return ORCGPU_OK;
}

// ... written to d_out (device, J.total bytes); asynchronous on the context's stream
int enc_emit(orcgpu_ctx* ctx, const EncJob& J, uint8_t* d_out) {
  if (!J.n_runs) return ORCGPU_OK;
  hipStream_t st = ctx->stream;
  if (J.kind == 0) {
    const uint64_t wgs = ((uint64_t)J.n_runs + 4ull * J.rpw - 1) / (4ull * J.rpw);
    ENC_TRY(launch(enc2_emit_kernel, wgs, true, 256, st, J.values, J.int_bytes, J.is_signed, (const EncRun*)J.recs, (const uint64_t*)J.offsets, J.n_runs, d_out, J.rpw,
                   J.d_n_runs));
  } else {
    ENC_TRY(launch(enc1_emit_kernel, ((uint64_t)J.n_runs + 255) / 256, true, 256, st, (const uint8_t*)J.values, (const uint16_t*)J.next16, (const uint32_t*)J.runs,
                   (const uint64_t*)J.offsets, J.n_runs, d_out, J.d_n_runs));
  }
  return ORCGPU_OK;
}

// one stream, from the caller's memory to the caller's memory
int enc_stream_call(orcgpu_ctx* ctx, int kind, const void* values, uint64_t n, uint64_t in_bytes, int int_bytes, int is_signed, uint32_t flags, uint8_t* out,
                    uint64_t out_cap, uint64_t* out_len, uint64_t n_bits = 0) {
  if (!ctx || (n && !values) || !out_len) return ORCGPU_INVALID_ARGUMENT;
  *out_len = 0;
  if (!n) return ORCGPU_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const bool on_device = flags & ORCGPU_ENC_ON_DEVICE;
  const void* d_values = values;
  if (!on_device) {
    if (!ctx->enc_in.ensure(in_bytes + kAlign)) {
      set_err(ctx, "encode: out of device memory (%llu bytes of values)", (unsigned long long)in_bytes);
      return ORCGPU_HIP_ERROR;
    }
    ENC_TRY(hipMemcpyAsync(ctx->enc_in.p, values, in_bytes, hipMemcpyHostToDevice, st));
    d_values = ctx->enc_in.p;
  }
  EncJob J;
  J.kind = kind;
  J.int_bytes = int_bytes;
  J.is_signed = is_signed;
  J.n = n;
  J.values = d_values;
  if (n_bits) {  // a bitmap: its bytes, bits reversed, are what the byte encoder sees (boolean.rs:157-169)
    if (!ctx->enc_tmp.ensure(n + kAlign)) {
      set_err(ctx, "encode: out of device memory");
      return ORCGPU_HIP_ERROR;
    }
    ENC_TRY(launch(enc_bool_bytes_kernel, n, false, 256, st, (const uint8_t*)d_values, n_bits, ctx->enc_tmp.p));
    J.values = ctx->enc_tmp.p;
  }
  int rc = enc_plan(ctx, J);
  if (rc) return rc;
  *out_len = J.total;
  if (!out) return ORCGPU_OK;  // the size is known now: the caller comes back with room for it
  if (out_cap < J.total) {
    set_err(ctx, "encode: the stream takes %llu bytes, the buffer holds %llu", (unsigned long long)J.total, (unsigned long long)out_cap);
    return ORCGPU_INVALID_ARGUMENT;
  }
  uint8_t* d_out = out;
  if (!on_device) {
    if (!ctx->enc_out[0].ensure(J.total + kAlign)) {
      set_err(ctx, "encode: out of device memory (%llu bytes of stream)", (unsigned long long)J.total);
      return ORCGPU_HIP_ERROR;
    }
    d_out = ctx->enc_out[0].p;
  }
  rc = enc_emit(ctx, J, d_out);
  if (rc) return rc;
  if (!on_device) ENC_TRY(hipMemcpyAsync(out, d_out, J.total, hipMemcpyDeviceToHost, st));
  ENC_TRY(hipStreamSynchronize(st));
  return ORCGPU_OK;
}

}  // namespace

extern "C" int orcgpu_encode_rle2(orcgpu_ctx* ctx, const void* values, uint64_t n, int int_bytes, int is_signed, uint32_t flags, uint8_t* out, uint64_t out_cap,
                                  uint64_t* out_len) {
  if (int_bytes != 2 && int_bytes != 4 && int_bytes != 8) return ORCGPU_INVALID_ARGUMENT;
  return enc_stream_call(ctx, 0, values, n, n * (uint64_t)int_bytes, int_bytes, is_signed ? 1 : 0, flags, out, out_cap, out_len);
}
extern "C" int orcgpu_encode_rle2_i64(orcgpu_ctx* ctx, const int64_t* values, uint64_t n, int is_signed, uint8_t* out, uint64_t out_cap, uint64_t* out_len) {
  return orcgpu_encode_rle2(ctx, values, n, 8, is_signed, 0, out, out_cap, out_len);
}
extern "C" int orcgpu_encode_byte_rle(orcgpu_ctx* ctx, const void* values, uint64_t n, uint32_t flags, uint8_t* out, uint64_t out_cap, uint64_t* out_len) {
  return enc_stream_call(ctx, 1, values, n, n, 1, 0, flags, out, out_cap, out_len);
}
extern "C" int orcgpu_encode_boolean(orcgpu_ctx* ctx, const void* bits, uint64_t n_bits, uint32_t flags, uint8_t* out, uint64_t out_cap, uint64_t* out_len) {
  const uint64_t nb = (n_bits + 7) / 8;
  return enc_stream_call(ctx, 1, bits, nb, nb, 1, 0, flags, out, out_cap, out_len, n_bits);
}

// ColumnStripeEncoder::{encode_array, finish} (writer/column.rs) for one array
extern "C" int orcgpu_encode_column(orcgpu_ctx* ctx, const orcgpu_enc_column* col, orcgpu_enc_stream streams[3], uint32_t* n_streams) {
  if (!ctx || !col || !streams || !n_streams) return ORCGPU_INVALID_ARGUMENT;
  *n_streams = 0;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  int elem = 0, offset_bytes = 0;  // bytes per fixed-width value (0: a bitmap / strings)
  bool is_string = false;
  switch (col->arrow_type) {
    case ORCGPU_ARROW_BOOLEAN: break;
    case ORCGPU_ARROW_INT8: elem = 1; break;
    case ORCGPU_ARROW_INT16: elem = 2; break;
    case ORCGPU_ARROW_INT32: case ORCGPU_ARROW_FLOAT32: elem = 4; break;
    case ORCGPU_ARROW_INT64: case ORCGPU_ARROW_FLOAT64: elem = 8; break;
    case ORCGPU_ARROW_UTF8: case ORCGPU_ARROW_BINARY: is_string = true; offset_bytes = 4; break;
    case ORCGPU_ARROW_LARGE_UTF8: case ORCGPU_ARROW_LARGE_BINARY: is_string = true; offset_bytes = 8; break;
    default:
      set_err(ctx, "encode: no column encoder for Arrow type %d (writer/stripe.rs:175-185)", col->arrow_type);
      return ORCGPU_UNSUPPORTED;
  }
  const uint64_t rows = col->n_rows;
  if (rows >= 0xffffffffull - 1024) return ORCGPU_INVALID_ARGUMENT;
  if (rows && (!col->values || (is_string && !col->offsets))) return ORCGPU_INVALID_ARGUMENT;
  const bool on_device = col->flags & ORCGPU_ENC_ON_DEVICE;
  const uint64_t vbytes = (rows + 7) / 8;
  // the array's buffers on the device
  const uint8_t* d_validity = col->validity;
  const uint8_t* d_values = (const uint8_t*)col->values;
  const uint8_t* d_offsets = (const uint8_t*)col->offsets;
  if (!on_device && rows) {
    uint64_t data_bytes = is_string ? 0 : (elem ? rows * (uint64_t)elem : vbytes);
    int64_t first = 0;
    if (is_string) {
      int64_t last;
      if (offset_bytes == 4) {
        first = ((const int32_t*)col->offsets)[0];
        last = ((const int32_t*)col->offsets)[rows];
      } else {
        first = ((const int64_t*)col->offsets)[0];
        last = ((const int64_t*)col->offsets)[rows];
      }
      if (first < 0 || last < first) return ORCGPU_INVALID_ARGUMENT;
      data_bytes = (uint64_t)last;  // (the bytes from 0: the offsets address them)
    }
    Bump I;
    const uint64_t o_val = I.take(col->validity ? vbytes : 0), o_data = I.take(data_bytes), o_off = I.take(is_string ? (rows + 1) * (uint64_t)offset_bytes : 0);
    if (!ctx->enc_in.ensure(I.off + kAlign)) {
      set_err(ctx, "encode: out of device memory (%llu bytes of input)", (unsigned long long)I.off);
      return ORCGPU_HIP_ERROR;
    }
    uint8_t* in = ctx->enc_in.p;
    if (col->validity) {
      ENC_TRY(hipMemcpyAsync(in + o_val, col->validity, vbytes, hipMemcpyHostToDevice, st));
      d_validity = in + o_val;
    }
    if (data_bytes) ENC_TRY(hipMemcpyAsync(in + o_data, col->values, data_bytes, hipMemcpyHostToDevice, st));
    d_values = in + o_data;
    if (is_string) {
      ENC_TRY(hipMemcpyAsync(in + o_off, col->offsets, (rows + 1) * (uint64_t)offset_bytes, hipMemcpyHostToDevice, st));
      d_offsets = in + o_off;
    }
  }
  // the valid rows: where each lands among them
  uint64_t n_valid = rows;
  const uint64_t n_words = (rows + 63) / 64;
  Bump T;
  const uint64_t o_wcnt = T.take(d_validity ? n_words * 4 : 0), o_woff = T.take(d_validity ? n_words * 8 : 0), o_sums = T.take((rows / 2048 + 2) * 8), o_tot = T.take(16);
  const uint64_t o_gather = T.take(rows * (uint64_t)(is_string ? offset_bytes : (elem ? elem : 1)));
  const uint64_t o_bits = T.take(vbytes + 8);
  const uint64_t o_vlen = T.take(is_string ? rows * 4 : 0), o_rowdst = T.take(is_string ? rows * 8 : 0);
  // (enc_tmp also serves enc_stream_call's reversed bitmap bytes: the column's PRESENT / Boolean streams keep theirs behind it)
  const uint64_t o_rev = T.take(vbytes + 8);
  if (!ctx->enc_tmp.ensure(T.off + kAlign)) {
    set_err(ctx, "encode: out of device memory (%llu bytes of gathered values)", (unsigned long long)T.off);
    return ORCGPU_HIP_ERROR;
  }
  uint8_t* tmp = ctx->enc_tmp.p;
  uint64_t* d_woff = (uint64_t*)(tmp + o_woff);
  if (d_validity && rows) {
    ENC_TRY(launch(enc_valid_counts_kernel, n_words, false, 256, st, d_validity, rows, (uint32_t*)(tmp + o_wcnt)));
    int rc = enc_scan(ctx, st, (const uint32_t*)(tmp + o_wcnt), n_words, (uint64_t*)(tmp + o_sums), (uint64_t*)(tmp + o_tot), d_woff);
    if (rc) return rc;
    ENC_TRY(hipMemcpyAsync(&n_valid, tmp + o_tot, 8, hipMemcpyDeviceToHost, st));
    ENC_TRY(hipStreamSynchronize(st));
  }
  uint32_t ns = 0;
  auto run_stream = [&](int slot, int kind, int stream_kind, const void* d_vals, uint64_t n, int int_bytes, int is_signed, uint64_t n_bits) -> int {
    EncJob J;
    J.kind = kind;
    J.int_bytes = int_bytes;
    J.is_signed = is_signed;
    J.n = n;
    J.values = d_vals;
    if (n_bits) {
      ENC_TRY(launch(enc_bool_bytes_kernel, n, false, 256, st, (const uint8_t*)d_vals, n_bits, tmp + o_rev));
      J.values = tmp + o_rev;
    }
    int rc = enc_plan(ctx, J);
    if (rc) return rc;
    if (!ctx->enc_out[slot].ensure(J.total + kAlign)) {
      set_err(ctx, "encode: out of device memory (%llu bytes of stream)", (unsigned long long)J.total);
      return ORCGPU_HIP_ERROR;
    }
    rc = enc_emit(ctx, J, ctx->enc_out[slot].p);
    if (rc) return rc;
    streams[ns].kind = stream_kind;
    streams[ns].pad = 0;
    streams[ns].data = ctx->enc_out[slot].p;
    streams[ns].len = J.total;
    ns++;
    return ORCGPU_OK;
  };
  int rc = ORCGPU_OK;
  if (col->arrow_type == ORCGPU_ARROW_BOOLEAN) {
    const uint8_t* bits = d_values;
    if (d_validity && rows) {  // the valid rows' values, as a bitmap again
      ENC_TRY(launch(enc_gather_valid_kernel, rows, false, 256, st, d_validity, rows, (const uint64_t*)d_woff, (const void*)d_values, 0, (void*)(tmp + o_gather)));
      ENC_TRY(launch(enc_bytes_to_bits_kernel, (n_valid + 7) / 8, false, 256, st, (const uint8_t*)(tmp + o_gather), n_valid, tmp + o_bits));
      bits = tmp + o_bits;
    }
    rc = run_stream(0, 1, 1, bits, (n_valid + 7) / 8, 1, 0, n_valid);
  } else if (!is_string) {
    const uint8_t* vals = d_values;
    if (d_validity && rows) {
      ENC_TRY(launch(enc_gather_valid_kernel, rows, false, 256, st, d_validity, rows, (const uint64_t*)d_woff, (const void*)d_values, elem, (void*)(tmp + o_gather)));
      vals = tmp + o_gather;
    }
    const bool is_float = col->arrow_type == ORCGPU_ARROW_FLOAT32 || col->arrow_type == ORCGPU_ARROW_FLOAT64;
    if (is_float) {  // FloatEncoder (encoding/float.rs:88-110): the values' bytes
      const uint64_t len = n_valid * (uint64_t)elem;
      if (!ctx->enc_out[0].ensure(len + kAlign)) return ORCGPU_HIP_ERROR;
      if (len) ENC_TRY(hipMemcpyAsync(ctx->enc_out[0].p, vals, len, hipMemcpyDeviceToDevice, st));
      streams[ns++] = orcgpu_enc_stream{1, 0, ctx->enc_out[0].p, len};
    } else if (elem == 1) {
      rc = run_stream(0, 1, 1, vals, n_valid, 1, 0, 0);
    } else {
      rc = run_stream(0, 0, 1, vals, n_valid, elem, 1, 0);
    }
  } else {
    // DATA: the valid rows' bytes; LENGTH: their lengths through RleV2Encoder<T::Offset, UnsignedEncoding> (column.rs:261-359)
    uint64_t data_len = 0;
    int64_t first = 0;
    if (rows) {
      uint32_t* d_bad = (uint32_t*)(tmp + o_tot + 8);  // (the second word of the scan's total: the scan writes the first only)
      ENC_TRY(hipMemsetAsync(d_bad, 0, 4, st));
      ENC_TRY(launch(enc_lengths_kernel, rows, false, 256, st, (const void*)d_offsets, offset_bytes, (const uint8_t*)d_validity, rows, (void*)(tmp + o_gather),
                     (uint32_t*)(tmp + o_vlen), d_bad));
      rc = enc_scan(ctx, st, (const uint32_t*)(tmp + o_vlen), rows, (uint64_t*)(tmp + o_sums), (uint64_t*)(tmp + o_tot), (uint64_t*)(tmp + o_rowdst));
      if (rc) return rc;
      ENC_TRY(hipMemcpyAsync(&data_len, tmp + o_tot, 8, hipMemcpyDeviceToHost, st));
      ENC_TRY(hipMemcpyAsync(&first, d_offsets, offset_bytes, hipMemcpyDeviceToHost, st));
      uint32_t bad_offsets = 0;
      ENC_TRY(hipMemcpyAsync(&bad_offsets, tmp + o_tot + 8, 4, hipMemcpyDeviceToHost, st));
      ENC_TRY(hipStreamSynchronize(st));
      if (bad_offsets || first < 0) {
        set_err(ctx, "encode: the column's offsets are not ascending (or a value is 4 GiB or longer)");
        return ORCGPU_INVALID_ARGUMENT;
      }
    }
    if (!ctx->enc_out[0].ensure(data_len + kAlign)) return ORCGPU_HIP_ERROR;
    if (data_len) {
      if (!d_validity) {
        ENC_TRY(hipMemcpyAsync(ctx->enc_out[0].p, d_values + first, data_len, hipMemcpyDeviceToDevice, st));
      } else {
        ENC_TRY(launch(enc_copy_strings_kernel, (rows + 3) / 4, true, 256, st, d_validity, (const void*)d_offsets, offset_bytes, rows, (const uint64_t*)(tmp + o_rowdst),
                       d_values, ctx->enc_out[0].p));
      }
    }
    streams[ns++] = orcgpu_enc_stream{1, 0, ctx->enc_out[0].p, data_len};
    // (the lengths of the valid rows stand gathered behind the lengths of all rows: enc_lengths_kernel wrote them per row;
    // with a bitmap they are gathered here)
    const uint8_t* lens = tmp + o_gather;
    if (d_validity && rows) {
      // gather in place is not possible: into the row-destination table's place, which the copy above has finished with (stream order)
      ENC_TRY(launch(enc_gather_valid_kernel, rows, false, 256, st, d_validity, rows, (const uint64_t*)d_woff, (const void*)(tmp + o_gather), offset_bytes,
                     (void*)(tmp + o_rowdst)));
      lens = tmp + o_rowdst;
    }
    if (rc == ORCGPU_OK) rc = run_stream(1, 0, 2, lens, n_valid, offset_bytes, 0, 0);
  }
  if (rc) return rc;
  // (GenericBinaryColumnEncoder::encode_array returns at once for an empty array, writer/column.rs:304-307: a string column of no
  // rows never gets a PRESENT stream, bitmap or not)
  if (col->validity && !(is_string && rows == 0)) rc = run_stream(2, 1, 0, d_validity, vbytes, 1, 0, rows);
  if (rc) return rc;
  ENC_TRY(hipStreamSynchronize(st));
  *n_streams = ns;
  return ORCGPU_OK;
}

extern "C" int orcgpu_encode_fetch(orcgpu_ctx* ctx, const orcgpu_enc_stream* stream, uint8_t* out) {
  if (!ctx || !stream || (stream->len && !out)) return ORCGPU_INVALID_ARGUMENT;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (stream->len) HIP_TRY(ctx, hipMemcpy(out, stream->data, stream->len, hipMemcpyDeviceToHost));
  return ORCGPU_OK;
}
