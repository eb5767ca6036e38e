// orcgpu_writer.inc -- ArrowWriterBuilder / ArrowWriter (src/arrow_writer.rs:34-156) over the device encoders of orcgpu_encode.inc:
// Arrow record batches (C Data Interface, host or device buffers) -> ORC files, byte for byte the reference's.
//
// What the writer holds on the device between calls, per column of the open stripe: the rows' presence (a byte each), the valid
// rows' values in the width the column's encoder takes them (Boolean: a byte each; strings: their lengths) and the strings' bytes.
// A stripe is encoded when it is flushed: every stream of every column through enc_plan / enc_emit, back to back in the stripe's
// stream order (writer/stripe.rs:128-150) in one device buffer, and brought to the host in one copy.
//
// The stripe cut (arrow_writer.rs:103-124: after every slice of batch_size rows, flush when the summed estimate exceeds
// stripe_byte_size) is computed, not replayed: the columns' estimates at every slice end follow from counts of valid values and
// bytes (wr_slice_counts_kernel) and, for the run-length encoded columns, from the run table of the stripe's values so far
// (wr_triggers_kernel: when each run is written out; wr_estimate_kernel: the bytes written out by each slice end).  Slices whose
// estimate cannot exceed the limit by an upper bound of the encoders' output are taken without that analysis; past them the
// analysed window grows geometrically.
//
// Compression (orcgpu_writer_set_compression; the reference writes CompressionKind::None only): after the last stream of a stripe
// is enqueued, every stream goes through the device compressor (orcgpu_compress.inc) from its slot into a slot of zout, in one
// launch set, before the first wait; the lengths that wait brings back are the compressed ones.  Stripe footers and the file
// Footer are written as original chunks.  The cut is unchanged: it is computed over the uncompressed encoders' estimates.
//
// Row index (orcgpu_writer_set_row_index; the reference writes none): each stripe is cut into row groups of `stride` rows.  The
// groups' ColumnStatistics come from one launch set over (column, group) jobs (device/col_stats.hip), enqueued before the
// stripe's streams; each stream's entry positions are searched in its encoder's run table right after its plan, while the table
// is alive; compressed files map them to chunk positions after the compressor.  Records, positions and the string minima /
// maxima come back with the stream lengths, in the same wait.  The host writes a ROW_INDEX stream per column (the root
// included) ahead of the data, the stripes' statistics as the Metadata section and the file's in the Footer.  Index bytes do
// not count toward the stripe cut.
//
// Bloom filters (orcgpu_writer_set_bloom_filter; the reference writes none): the listed columns' bitsets, one per row group, are
// built behind the statistics kernels from the same tables (device/bloom_build.hip) and come back in the same copy; the host
// writes a BLOOM_FILTER_UTF8 stream behind the column's ROW_INDEX.
//
// The files: orcgpu_writer_host.inc -- everything that never touches the device (the column tree, the description of a column's
// streams, statistics, the bytes of index streams, footers and the tail); this file -- the writer, its device buffers, the
// stream emitters and the C ABI; orcgpu_writer_flush.inc -- a stripe flushed (wr_dictionaries, wr_flush);
// orcgpu_writer_write.inc -- a batch taken in and the stripe cut (wr_write).
namespace {

// the buffer keeps its contents when it grows (stream-ordered copy)
struct DevVec {
  uint8_t* p = nullptr;
  size_t cap = 0;
  bool reserve(size_t n, size_t used, hipStream_t st) {
    if (n <= cap) return true;
    size_t want = std::max<size_t>(n + n / 2, 1u << 16);
    uint8_t* q = nullptr;
    if (hipMalloc((void**)&q, want) != hipSuccess) return false;
    if (used && hipMemcpyAsync(q, p, used, hipMemcpyDeviceToDevice, st) != hipSuccess) return false;
    if (p) {
      (void)hipStreamSynchronize(st);
      (void)hipFree(p);
    }
    p = q;
    cap = want;
    return true;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// a column's device buffers (its description: WrCol, orcgpu_writer_host.inc)
struct WrColDev {
  // what the open stripe holds: the rows' presence, the valid rows' values, the strings' bytes.  vals2: the second value stream's
  // values -- Timestamp: the nanosecond codes (u64; vals: the stored seconds); Decimal128: the scale once per valid value (i16;
  // vals: the values themselves, kept only with a row index, for its statistics; data: their varints)
  DevVec pres, vals, vals2, data;
  // this write call's batch, in the same form
  DevBuf b_bits, b_pres, b_vals, b_vals2, b_data, b_tmp;
  // nested: a Struct's / List's children's rows as a map (device/writer_nested.hip); a leaf's arrays gathered through its parent's
  DevBuf k_map, b_gath;
  // dictionary: the tables of device/writer_dict.hip (ids, entry lengths and bytes at these offsets of b_dict)
  uint64_t o_dict_ids = 0, o_dict_len = 0, o_dict_data = 0;
  DevBuf b_dict;
  const uint8_t* src(int s) const {  // WrSrc
    switch (s) {
      case WR_SRC_VALS: return vals.p;
      case WR_SRC_VALS2: return vals2.p;
      case WR_SRC_DATA: return data.p;
      case WR_SRC_PRES: return pres.p;
      case WR_SRC_DICT_IDS: return b_dict.p + o_dict_ids;
      case WR_SRC_DICT_LEN: return b_dict.p + o_dict_len;
      default: return b_dict.p + o_dict_data;
    }
  }
  void release() {
    for (DevVec* v : {&pres, &vals, &vals2, &data}) v->release();
    for (DevBuf* b : {&b_bits, &b_pres, &b_vals, &b_vals2, &b_data, &b_tmp, &k_map, &b_gath, &b_dict}) b->release();
  }
};

}  // namespace

struct orcgpu_writer {
  orcgpu_ctx* ctx = nullptr;
  FILE* f = nullptr;
  bool to_memory = false;
  std::vector<uint8_t> mem;  // the memory sink's bytes not drained yet
  bool closed = false, failed = false;
  uint64_t batch_size = 1024, stripe_byte_size = 64ull << 20;
  std::vector<WrCol> cols;  // every column of the tree but the root, preorder
  std::vector<WrColDev> dev;  // ... and its device buffers
  std::vector<int> root_kids;
  bool nested = false;      // a Struct, List or Map column among them
  uint64_t nested_slices = 0, nested_gathers = 0;  // columns of a write taken as a slice of their array / gathered through a map
  DevBuf nest;              // a write's NestRows per column, `bad`, and the columns' slice ends
  std::vector<WrField> fields;
  std::string root_metadata;
  int64_t root_flags = 0;
  uint64_t written = 3;  // bytes in the file so far ("ORC")
  uint64_t rows = 0;     // of the open stripe (StripeWriter::row_count)
  std::vector<WrStripe> stripes;
  uint64_t round_trips = 0, stripe_round_trips = 0, window_hint = 16;
  DevBuf slice_counts, est, trig, lens, bits;
  uint64_t bits_at = 0;
  DevVec out, slots;
  // what the size analysis knows exactly: the run-length encoded columns' summed estimate when each column had base_valid values
  uint64_t base_rle = 0;
  uint8_t* pinned = nullptr;
  size_t pinned_cap = 0;
  // compression (orcgpu_writer_set_compression): the streams' chunks in zout, a slot each; `started` once write / flush / close ran
  int comp = ORCGPU_COMP_NONE;
  uint64_t comp_block = kLzcDefaultBlock;
  bool started = false;
  DevVec zout;
  // row index (orcgpu_writer_set_row_index): 0 = none; the device tables of a stripe's index and the records' copy on the host
  uint64_t stride = 0;
  DevVec ix;
  uint8_t* ix_pinned = nullptr;
  size_t ix_pinned_cap = 0;
  std::vector<std::vector<WrStat>> stripe_stats;  // [stripe][column], column 0 the root
  // dictionary (orcgpu_writer_set_dictionary): the key size threshold (0: every string column DIRECT_V2), the bits of the hash
  // that are used (ORCGPU_DICT_HASH_BITS), what a stripe's columns bring back, and the (string column, stripe) pairs so far
  double dict_threshold = 0.0;
  uint32_t dict_hash_mask = 0xffffffffu;
  DevBuf dict_res;
  uint64_t n_dictionary = 0, n_direct = 0;
  // Bloom filters (orcgpu_writer_set_bloom_filter): the listed columns (WrCol::bloom), n_bloom of them; every filter's 64-bit
  // words and hash functions, sized once from the stride and the false positive probability
  uint64_t n_bloom = 0, bloom_words = 0;
  uint32_t bloom_k = 0;
};

namespace {

#define WR_TRY(expr)                                                                                    \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) {                                                                             \
      set_err(ctx, "writer: %s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return ORCGPU_HIP_ERROR;                                                                          \
    }                                                                                                   \
  } while (0)

int wr_sync(orcgpu_writer* w) {
  orcgpu_ctx* ctx = w->ctx;
  w->round_trips++;
  WR_TRY(hipStreamSynchronize(ctx->stream));
  return ORCGPU_OK;
}

int wr_sink(orcgpu_writer* w, const uint8_t* p, size_t n) {
  if (!n) return ORCGPU_OK;
  if (w->to_memory) {
    w->mem.insert(w->mem.end(), p, p + n);
  } else if (fwrite(p, 1, n, w->f) != n) {
    set_err(w->ctx, "writer: cannot write %zu bytes", n);
    return ORCGPU_IO_ERROR;
  }
  w->written += n;
  return ORCGPU_OK;
}

// the schema's columns and the options (the sink is the caller's)
int wr_prepare(orcgpu_ctx* ctx, const ArrowSchema* schema, const orcgpu_writer_opts* opts, orcgpu_writer* w) {
  w->ctx = ctx;
  std::string err;
  int rc = wr_read_schema(err, schema, w->fields, w->root_metadata, w->root_flags);
  WrTree t;
  if (!rc) rc = wr_tree_of(err, w->fields, t);
  if (rc) {
    if (!err.empty()) set_err(ctx, "%s", err.c_str());
    return rc;
  }
  w->cols = std::move(t.cols);
  w->root_kids = std::move(t.root_kids);
  w->nested = t.nested;
  w->dev.resize(w->cols.size());
  if (opts && opts->batch_size) w->batch_size = opts->batch_size;
  if (opts && opts->stripe_byte_size) w->stripe_byte_size = opts->stripe_byte_size;
  // ORCGPU_DICT_HASH_BITS=N (1 .. 32): the bits of a string's hash the dictionary tables use -- few bits make long probe
  // sequences of small inputs; the file's bytes do not depend on it
  if (const char* e = getenv("ORCGPU_DICT_HASH_BITS")) {
    const int bits = atoi(e);
    if (bits >= 1 && bits <= 32) w->dict_hash_mask = bits == 32 ? 0xffffffffu : (1u << bits) - 1;
  }
  return ORCGPU_OK;
}

// ArrowWriterBuilder::try_build: the magic "ORC" first (arrow_writer.rs:73-75)
int wr_start(std::unique_ptr<orcgpu_writer>& w, orcgpu_writer** out) {
  static const uint8_t magic[3] = {'O', 'R', 'C'};
  w->written = 0;
  int rc = wr_sink(w.get(), magic, 3);
  if (rc) return rc;
  *out = w.release();
  return ORCGPU_OK;
}

// DevBuf::ensure waits for the device when it grows (hipFree): counted
bool wr_ensure(orcgpu_writer* w, DevBuf& b, uint64_t n) {
  if (n > b.cap) w->round_trips++;
  return b.ensure(n);
}
bool wr_reserve(orcgpu_writer* w, DevVec& v, uint64_t n, uint64_t used) {
  if (n > v.cap && v.p) w->round_trips++;
  return v.reserve(n, used, w->ctx->stream);
}

// pinned host memory of at least n bytes (what it held is gone).  hipHostFree waits for the device: counted; count_fresh: the
// first allocation is counted as well (hipHostMalloc)
int wr_pinned(orcgpu_writer* w, uint8_t*& p, size_t& cap, size_t n, bool count_fresh) {
  orcgpu_ctx* ctx = w->ctx;
  if (n <= cap) return ORCGPU_OK;
  if (p || count_fresh) w->round_trips++;
  if (p) (void)hipHostFree(p);
  p = nullptr;
  cap = 0;
  WR_TRY(hipHostMalloc((void**)&p, n + n / 2, 0));
  cap = n + n / 2;
  return ORCGPU_OK;
}

// a stream's row index positions (ix_pos_kernel): where group g starts, into pos[g * 4 ..]
struct WrIxPos {
  int mode;                    // ix_pos_kernel's
  uint64_t G, S, n;            // groups, stride, values of the stream (bit streams: bits)
  const uint64_t* vscan;       // the column's first values per group
  const uint64_t* bscan;       // ... first string bytes
  int elem;
  uint64_t* pos;
};
hipError_t wr_ix_pos(orcgpu_ctx* ctx, const WrIxPos* ip, const EncJob* J) {
  if (!ip || !ip->G) return hipSuccess;
  const bool runs = J && J->n_runs;
  return launch(ix_pos_kernel, ip->G, false, 256, ctx->stream, ip->mode, ip->G, ip->S, ip->vscan, ip->bscan, runs ? ip->n : (uint64_t)0, ip->elem,
                runs ? (const uint32_t*)J->runs : (const uint32_t*)nullptr, runs ? (const uint64_t*)J->offsets : (const uint64_t*)nullptr,
                runs ? J->d_n_runs : (const uint64_t*)nullptr, runs ? J->d_total : (const uint64_t*)nullptr, ip->pos);
}

// one stream of the stripe, enqueued: values (device) through the encoder into the slot at *at of w->slots (room: its bound);
// its length lands in d_lens[li] on the device.  ip: its row index positions, searched while the run table is the stream's
int wr_rle_stream(orcgpu_writer* w, int enc, const void* d_values, uint64_t n, int int_bytes, int is_signed, uint64_t* at, uint64_t li,
                  const WrIxPos* ip = nullptr) {
  orcgpu_ctx* ctx = w->ctx;
  uint64_t* d_lens = (uint64_t*)w->lens.p;
  if (!n) {
    WR_TRY(hipMemsetAsync(d_lens + li, 0, 8, ctx->stream));
    WR_TRY(wr_ix_pos(ctx, ip, nullptr));
    return ORCGPU_OK;
  }
  EncJob J;
  J.kind = enc == WR_ENC_BYTE_RLE ? 1 : 0;
  J.int_bytes = int_bytes;
  J.is_signed = is_signed;
  J.n = n;
  J.values = d_values;
  J.deferred = true;
  J.syncs = &w->round_trips;
  int rc = enc_plan(ctx, J);
  if (rc) return rc;
  const uint64_t room = wr_stream_bound(enc, int_bytes, n);
  if (!wr_reserve(w, w->slots, *at + room + kAlign, *at)) {
    set_err(ctx, "writer: out of device memory (%llu bytes of stripe)", (unsigned long long)(*at + room));
    return ORCGPU_HIP_ERROR;
  }
  rc = enc_emit(ctx, J, w->slots.p + *at);
  if (rc) return rc;
  WR_TRY(hipMemcpyAsync(d_lens + li, J.d_total, 8, hipMemcpyDeviceToDevice, ctx->stream));
  WR_TRY(wr_ix_pos(ctx, ip, &J));
  *at += align_up(room);
  return ORCGPU_OK;
}

// a bitmap of n bits given as 0 / 1 bytes through BooleanEncoder (boolean.rs:157-169)
int wr_bool_stream(orcgpu_writer* w, const uint8_t* d_bytes, uint64_t n, uint64_t* at, uint64_t li, const WrIxPos* ip = nullptr) {
  orcgpu_ctx* ctx = w->ctx;
  const uint64_t nb = (n + 7) / 8;
  // (the bitmaps of every Boolean / PRESENT stream of the stripe stay until it is written: one region each, at *at of `bits`)
  const uint64_t o = w->bits_at;
  w->bits_at += align_up(2 * nb + 16);
  if (w->bits_at > w->bits.cap) return ORCGPU_UNEXPECTED;
  uint8_t* bits = w->bits.p + o;
  uint8_t* rev = bits + align_up(nb + 8);
  WR_TRY(launch(enc_bytes_to_bits_kernel, nb, false, 256, ctx->stream, d_bytes, n, bits));
  WR_TRY(launch(enc_bool_bytes_kernel, nb, false, 256, ctx->stream, (const uint8_t*)bits, n, rev));
  return wr_rle_stream(w, WR_ENC_BYTE_RLE, rev, nb, 1, 0, at, li, ip);
}

// DATA of floats and strings: the bytes themselves (the length is known on the host)
int wr_copy_stream(orcgpu_writer* w, const uint8_t* d_src, uint64_t n, uint64_t* at, uint64_t li, std::vector<uint64_t>& known) {
  orcgpu_ctx* ctx = w->ctx;
  if (!wr_reserve(w, w->slots, *at + n + kAlign, *at)) return ORCGPU_HIP_ERROR;
  if (n) WR_TRY(hipMemcpyAsync(w->slots.p + *at, d_src, n, hipMemcpyDeviceToDevice, ctx->stream));
  known[li] = n;
  *at += align_up(n);
  return ORCGPU_OK;
}

constexpr uint64_t kBloomMaxWords = 1ull << 27;  // a row group's Bloom filter: at most 2^30 bytes

int wr_flush(orcgpu_writer* w);
int wr_write(orcgpu_writer* w, const struct ArrowArray* batch, uint32_t flags, const std::vector<int64_t>& dev_ends, bool* rejected);

// the tail: Footer, PostScript, the PostScript's length
int wr_close(orcgpu_writer* w) {
  const std::vector<uint8_t> tail = wr_tail(w->cols, w->root_kids, w->stripes, w->stripe_stats, w->stride, w->comp, w->comp_block);
  return wr_sink(w, tail.data(), tail.size());
}

// what every array of a batch is asked before its buffers are looked at: the buffers its column's type has
bool wr_array_ok(const WrCol& c, const ArrowArray* a) {
  const int need = c.stream_kind == WR_STRUCT ? 1 : (c.is_string ? 3 : 2);
  return a && a->offset >= 0 && a->n_buffers >= need && a->buffers;
}

}  // namespace

extern "C" int orcgpu_writer_open_file(orcgpu_ctx* ctx, const char* path, const struct ArrowSchema* schema, const orcgpu_writer_opts* opts, orcgpu_writer** out) {
  if (!ctx || !path || !schema || !out) return ORCGPU_INVALID_ARGUMENT;
  *out = nullptr;
  auto w = std::make_unique<orcgpu_writer>();
  int rc = wr_prepare(ctx, schema, opts, w.get());
  if (rc) return rc;
  w->f = fopen(path, "wb");
  if (!w->f) {
    set_err(ctx, "writer: cannot create '%s'", path);
    return ORCGPU_IO_ERROR;
  }
  rc = wr_start(w, out);
  if (rc) fclose(w->f);
  return rc;
}

extern "C" int orcgpu_writer_open_bytes(orcgpu_ctx* ctx, const struct ArrowSchema* schema, const orcgpu_writer_opts* opts, orcgpu_writer** out) {
  if (!ctx || !schema || !out) return ORCGPU_INVALID_ARGUMENT;
  *out = nullptr;
  auto w = std::make_unique<orcgpu_writer>();
  w->to_memory = true;
  int rc = wr_prepare(ctx, schema, opts, w.get());
  return rc ? rc : wr_start(w, out);
}

// everything that can reject the batch is checked before the writer changes; a failure after that leaves it failed
extern "C" int orcgpu_writer_write(orcgpu_writer* w, const struct ArrowSchema* schema, const struct ArrowArray* batch, uint32_t flags) {
  if (!w || !schema || !batch || w->closed) return ORCGPU_INVALID_ARGUMENT;
  if (w->failed) return ORCGPU_UNEXPECTED;
  w->started = true;
  orcgpu_ctx* ctx = w->ctx;
  {  // ensure!(batch.schema() == self.schema, Unexpected)
    std::vector<WrField> fields;
    std::string md;
    int64_t fl;
    std::string err;
    int rc = wr_read_schema(err, schema, fields, md, fl);
    bool same = rc == ORCGPU_OK && md == w->root_metadata && fields.size() == w->fields.size();
    for (size_t i = 0; same && i < fields.size(); i++) same = fields[i].same(w->fields[i]);
    if (!same) {
      set_err(ctx, "writer: RecordBatch doesn't match expected schema");
      return ORCGPU_UNEXPECTED;
    }
  }
  const int64_t R = batch->length;
  const size_t nc = w->cols.size(), nr = w->root_kids.size();
  if (R < 0 || batch->n_children != (int64_t)nr || (nr && !batch->children)) return ORCGPU_INVALID_ARGUMENT;
  if (w->nested && (flags & ORCGPU_ENC_ON_DEVICE)) {
    set_err(ctx, "writer: batches in device memory (ORCGPU_ENC_ON_DEVICE) are not taken by a writer whose schema has a Struct, List or Map column");
    return ORCGPU_UNSUPPORTED;
  }
  std::vector<int64_t> dev_ends(2 * nc, 0);
  if (R > 0) {
    const bool on_device = flags & ORCGPU_ENC_ON_DEVICE;
    bool any_device_strings = false;
    for (size_t ci = 0; ci < nc; ci++) {
      const WrCol& c = w->cols[ci];
      if (c.parent >= 0) continue;  // (the columns below: checked as the write walks the tree, before anything changes)
      const ArrowArray* a = batch->children[c.child];
      if (c.is_nest()) {
        if (wr_array_ok(c, a) && batch->offset >= 0 && a->length >= batch->offset + R) continue;
        set_err(ctx, "writer: column %zu of the batch is not an Arrow array of its type", ci);
        return ORCGPU_INVALID_ARGUMENT;
      }
      if (!wr_array_ok(c, a) || batch->offset < 0 || a->length < batch->offset + R || !a->buffers[1] || (c.is_string && !a->buffers[2])) {
        set_err(ctx, "writer: column %zu of the batch is not an Arrow array of its type", ci);
        return ORCGPU_INVALID_ARGUMENT;
      }
      if (!c.is_string) continue;
      const uint64_t off = (uint64_t)(batch->offset + a->offset);
      const uint8_t* o = (const uint8_t*)a->buffers[1];
      if (on_device) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        WR_TRY(hipMemcpyAsync(&dev_ends[2 * ci], o + off * c.elem, c.elem, hipMemcpyDeviceToHost, ctx->stream));
        WR_TRY(hipMemcpyAsync(&dev_ends[2 * ci + 1], o + (off + R) * c.elem, c.elem, hipMemcpyDeviceToHost, ctx->stream));
        any_device_strings = true;
        continue;
      }
      // host offsets: ascending (they bound the bytes the copy writes)
      bool ascending = (c.elem == 4 ? (int64_t)((const int32_t*)o)[off] : ((const int64_t*)o)[off]) >= 0;
      for (uint64_t r = off; ascending && r < off + (uint64_t)R; r++)
        ascending = c.elem == 4 ? ((const int32_t*)o)[r] <= ((const int32_t*)o)[r + 1] : ((const int64_t*)o)[r] <= ((const int64_t*)o)[r + 1];
      if (!ascending) {
        set_err(ctx, "writer: the offsets of column %zu are not ascending", ci);
        return ORCGPU_INVALID_ARGUMENT;
      }
    }
    if (any_device_strings) {  // one wait for every string column's first and last offset
      int rc = wr_sync(w);
      if (rc) return rc;
      for (size_t ci = 0; ci < nc; ci++) {
        if (!w->cols[ci].is_string) continue;
        if (w->cols[ci].elem == 4) {
          dev_ends[2 * ci] = (int32_t)dev_ends[2 * ci];
          dev_ends[2 * ci + 1] = (int32_t)dev_ends[2 * ci + 1];
        }
        if (dev_ends[2 * ci] < 0 || dev_ends[2 * ci + 1] < dev_ends[2 * ci]) {
          set_err(ctx, "writer: the offsets of column %zu are not ascending", ci);
          return ORCGPU_INVALID_ARGUMENT;
        }
      }
    }
  }
  bool rejected = false;
  int rc = wr_write(w, batch, flags, dev_ends, &rejected);
  if (rc && !rejected) w->failed = true;
  return rc;
}

extern "C" int orcgpu_writer_flush_stripe(orcgpu_writer* w) {
  if (!w || w->closed) return ORCGPU_INVALID_ARGUMENT;
  if (w->failed) return ORCGPU_UNEXPECTED;
  w->started = true;
  HIP_TRY(w->ctx, hipSetDevice(w->ctx->device));
  int rc = wr_flush(w);
  if (rc) w->failed = true;
  return rc;
}

extern "C" int orcgpu_writer_set_compression(orcgpu_writer* w, int kind, uint64_t block_size) {
  if (!w) return ORCGPU_INVALID_ARGUMENT;
  if (kind == ORCGPU_COMP_ZLIB || kind == ORCGPU_COMP_LZO || kind == ORCGPU_COMP_ZSTD) {
    set_err(w->ctx, "writer: only Snappy and LZ4 files are written compressed");
    return ORCGPU_UNSUPPORTED;
  }
  const uint64_t B = block_size ? block_size : kLzcDefaultBlock;
  if ((kind != ORCGPU_COMP_NONE && lzc_codec(kind) < 0) || B > kLzcMaxBlock) return ORCGPU_INVALID_ARGUMENT;
  if (w->started || w->closed) {
    set_err(w->ctx, "writer: the compression is set before the first write, flush_stripe or close");
    return ORCGPU_INVALID_ARGUMENT;
  }
  w->comp = kind;
  w->comp_block = B;
  return ORCGPU_OK;
}

extern "C" int orcgpu_writer_set_dictionary(orcgpu_writer* w, double key_size_threshold) {
  if (!w) return ORCGPU_INVALID_ARGUMENT;
  if (!(key_size_threshold >= 0.0 && key_size_threshold <= 1.0)) {  // (NaN fails both)
    set_err(w->ctx, "writer: the dictionary key size threshold is 0 (no dictionaries) or in (0, 1]");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (w->started || w->closed) {
    set_err(w->ctx, "writer: the dictionary key size threshold is set before the first write, flush_stripe or close");
    return ORCGPU_INVALID_ARGUMENT;
  }
  w->dict_threshold = key_size_threshold;
  return ORCGPU_OK;
}

extern "C" int orcgpu_writer_dictionary_counts(const orcgpu_writer* w, uint64_t* dictionary, uint64_t* direct) {
  if (!w || !dictionary || !direct) return ORCGPU_INVALID_ARGUMENT;
  *dictionary = w->n_dictionary;
  *direct = w->n_direct;
  return ORCGPU_OK;
}

extern "C" int orcgpu_writer_set_row_index(orcgpu_writer* w, uint64_t stride) {
  if (!w) return ORCGPU_INVALID_ARGUMENT;
  if (stride > 0x7fffffffull) {
    set_err(w->ctx, "writer: the row index stride is 0 (none) or 1 .. 2^31 - 1");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (w->started || w->closed) {
    set_err(w->ctx, "writer: the row index is set before the first write, flush_stripe or close");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (stride && w->nested) {
    set_err(w->ctx, "writer: no row index for a schema with a Struct, List or Map column (the row groups of their children are not written)");
    return ORCGPU_UNSUPPORTED;
  }
  if (w->n_bloom) {
    set_err(w->ctx, "writer: the row index stride is set before the Bloom filters, which are sized from it");
    return ORCGPU_INVALID_ARGUMENT;
  }
  w->stride = stride;
  return ORCGPU_OK;
}

extern "C" int orcgpu_writer_set_bloom_filter(orcgpu_writer* w, const char* const* columns, uint32_t n_columns, double fpp) {
  if (!w || (n_columns && !columns)) return ORCGPU_INVALID_ARGUMENT;
  orcgpu_ctx* ctx = w->ctx;
  if (w->started || w->closed) {
    set_err(ctx, "writer: the Bloom filters are set before the first write, flush_stripe or close");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (!w->stride) {
    set_err(ctx, "writer: Bloom filters need a row index (orcgpu_writer_set_row_index with a stride above 0 first): there is one per row group");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (!(fpp > 0.0 && fpp < 1.0)) {  // (NaN fails both)
    set_err(ctx, "writer: the Bloom filters' false positive probability is strictly between 0 and 1");
    return ORCGPU_INVALID_ARGUMENT;
  }
  std::vector<size_t> listed;
  for (uint32_t i = 0; i < n_columns; i++) {
    if (!columns[i]) return ORCGPU_INVALID_ARGUMENT;
    size_t at = w->cols.size();
    for (int k : w->root_kids)
      if (w->cols[(size_t)k].name == columns[i]) at = (size_t)k;
    if (at == w->cols.size()) {
      set_err(ctx, "writer: no field '%s' for a Bloom filter (a top-level field's name)", columns[i]);
      return ORCGPU_INVALID_ARGUMENT;
    }
    if (std::find(listed.begin(), listed.end(), at) != listed.end()) {
      set_err(ctx, "writer: field '%s' is listed twice for a Bloom filter", columns[i]);
      return ORCGPU_INVALID_ARGUMENT;
    }
    const int kind = w->cols[at].stream_kind;
    if (kind != WR_INT && kind != WR_BYTE && kind != WR_FLOAT && kind != WR_STRING) {
      set_err(ctx, "writer: no Bloom filter for field '%s': Boolean, Timestamp and Decimal128 columns get none (integers, floats, strings and binaries do)",
              columns[i]);
      return ORCGPU_UNSUPPORTED;
    }
    listed.push_back(at);
  }
  uint64_t words = 0;
  uint32_t k = 0;
  wr_bloom_size(w->stride, fpp, words, k);
  if (n_columns && words > kBloomMaxWords) {
    set_err(ctx, "writer: a Bloom filter of %llu bytes per row group (at most 2^30: a larger stride or probability)", (unsigned long long)words * 8);
    return ORCGPU_INVALID_ARGUMENT;
  }
  for (auto& c : w->cols) c.bloom = false;
  for (size_t at : listed) w->cols[at].bloom = true;
  w->n_bloom = listed.size();
  w->bloom_words = words;
  w->bloom_k = k;
  return ORCGPU_OK;
}

extern "C" int orcgpu_writer_close(orcgpu_writer* w) {
  if (!w || w->closed) return ORCGPU_INVALID_ARGUMENT;
  if (w->failed) return ORCGPU_UNEXPECTED;
  w->started = true;
  HIP_TRY(w->ctx, hipSetDevice(w->ctx->device));
  int rc = ORCGPU_OK;
  if (w->rows > 0) rc = wr_flush(w);
  if (!rc) rc = wr_close(w);
  w->closed = true;
  if (w->f) {
    if (fclose(w->f) != 0 && !rc) rc = ORCGPU_IO_ERROR;
    w->f = nullptr;
  }
  return rc;
}

extern "C" int orcgpu_writer_take_bytes(orcgpu_writer* w, uint8_t* out, uint64_t cap, uint64_t* len) {
  if (!w || !len || !w->to_memory) return ORCGPU_INVALID_ARGUMENT;
  *len = w->mem.size();
  if (!out) return ORCGPU_OK;
  if (cap < w->mem.size()) return ORCGPU_INVALID_ARGUMENT;
  if (!w->mem.empty()) memcpy(out, w->mem.data(), w->mem.size());
  w->mem.clear();
  return ORCGPU_OK;
}

extern "C" int orcgpu_writer_stats(const orcgpu_writer* w, orcgpu_writer_counts* out) {
  if (!w || !out) return ORCGPU_INVALID_ARGUMENT;
  out->stripes = w->stripes.size();
  uint64_t rows = 0;
  for (auto& s : w->stripes) rows += s.rows;
  out->rows = rows;
  out->bytes = w->written;
  out->round_trips = w->round_trips;
  out->stripe_round_trips = w->stripe_round_trips;
  out->nested_slices = w->nested_slices;
  out->nested_gathers = w->nested_gathers;
  return ORCGPU_OK;
}

extern "C" uint64_t orcgpu_writer_stripe_rows(const orcgpu_writer* w, uint64_t stripe) {
  return w && stripe < w->stripes.size() ? w->stripes[stripe].rows : 0;
}

extern "C" void orcgpu_writer_free(orcgpu_writer* w) {
  if (!w) return;
  if (w->f) fclose(w->f);
  if (w->ctx) (void)hipSetDevice(w->ctx->device);
  if (w->ctx) (void)hipStreamSynchronize(w->ctx->stream);
  for (auto& d : w->dev) d.release();
  w->nest.release();
  w->slice_counts.release();
  w->est.release();
  w->trig.release();
  w->lens.release();
  w->bits.release();
  w->out.release();
  w->slots.release();
  w->zout.release();
  w->ix.release();
  w->dict_res.release();
  if (w->pinned) (void)hipHostFree(w->pinned);
  if (w->ix_pinned) (void)hipHostFree(w->ix_pinned);
  delete w;
}
