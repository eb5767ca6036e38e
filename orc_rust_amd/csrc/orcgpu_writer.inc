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

// a protobuf message being written: the fields in the order they are added (prost writes them in declaration order)
struct PbOut {
  std::vector<uint8_t> b;
  void varint(uint64_t v) {
    while (v >= 0x80) {
      b.push_back((uint8_t)(v | 0x80));
      v >>= 7;
    }
    b.push_back((uint8_t)v);
  }
  void key(uint32_t field, uint32_t wire) { varint(((uint64_t)field << 3) | wire); }
  void u64(uint32_t field, uint64_t v) {
    key(field, 0);
    varint(v);
  }
  void bytes(uint32_t field, const void* p, size_t n) {
    key(field, 2);
    varint(n);
    b.insert(b.end(), (const uint8_t*)p, (const uint8_t*)p + n);
  }
  void msg(uint32_t field, const PbOut& m) { bytes(field, m.b.data(), m.b.size()); }
  void sint(uint32_t field, int64_t v) { u64(field, ((uint64_t)v << 1) ^ (uint64_t)(v >> 63)); }
  void f64(uint32_t field, double v) {
    key(field, 1);
    uint8_t x[8];
    memcpy(x, &v, 8);
    b.insert(b.end(), x, x + 8);
  }
  void packed(uint32_t field, const std::vector<uint64_t>& v) {  // [packed = true]: nothing at all when empty
    if (v.empty()) return;
    PbOut m;
    for (uint64_t x : v) m.varint(x);
    bytes(field, m.b.data(), m.b.size());
  }
};

struct WrStripe {
  uint64_t offset, data_length, footer_length, rows, index_length;
};

// ColumnStatistics of a range of rows of one column, as the device's records and the host's merges hold them
struct WrStat {
  uint64_t count = 0, bytes = 0, trues = 0;
  bool has_null = false, has_nan = false;
  int64_t imin = 0, imax = 0;
  __int128 isum = 0;  // exact: written when it fits in i64
  double dmin = 0, dmax = 0, dsum = 0, dsum_lo = 0;
  double dbig = 0, dbig_lo = 0;  // the sum of the values of magnitude >= 2^960, scaled by 2^-64 (col_stats.hip: IX_BIG)
  std::string smin, smax;          // their first IX_STR_KEEP bytes at most
  uint64_t smin_len = 0, smax_len = 0;  // and their whole lengths
  uint32_t nmin = 0, nmax = 0;     // Timestamp: the nanoseconds of the minimum / maximum (imin / imax: their seconds)
  __int128 qmin = 0, qmax = 0;     // Decimal128
  uint64_t qsum[4] = {0, 0, 0, 0};  // ... the exact sum, 256 bits, two's complement
};

struct WrCol {
  int elem = 0;        // bytes of a value as the column's value encoder takes it (Boolean: a byte; strings: the offset width)
  bool is_string = false;
  int stream_kind = 0; // 0 Integer RLE v2 (signed), 1 byte RLE, 2 raw floats, 3 Boolean, 4 strings (bytes + unsigned RLE v2 lengths),
                       // 5 Timestamp (seconds + nanosecond codes, RLE v2), 6 Decimal128 (varint bytes + the scale, signed RLE v2),
                       // 7 Struct (PRESENT alone), 8 List / Map (vals: the valid rows' lengths, unsigned RLE v2, in the offsets' width)
  int orc_kind = 0;    // Type.Kind
  int encoding = 0;    // ColumnEncoding.Kind
  std::string name, path;
  // the column tree, preorder (column id = index + 1): the parent's index (-1: the root), which of the parent array's children
  // the column's array is (a Map's: of its entries struct's), and the children's indexes
  int parent = -1, child = 0;
  std::vector<int> kids;
  bool present = false;  // sticky once an array with a validity bitmap arrived (writer/column.rs:103-139)
  uint64_t rows = 0, n_valid = 0, n_bytes = 0;  // of the open stripe
  uint64_t base_valid = 0;                       // values of the stripe when orcgpu_writer::base_rle was found
  int64_t ups = 1, npu = 1;         // Timestamp: units per second, nanoseconds per unit
  uint32_t precision = 0, scale = 0;  // Decimal128
  // vals2: the second value stream's values -- Timestamp: the nanosecond codes (u64; vals: the stored seconds); Decimal128: the
  // scale once per valid value (i16; vals: the values themselves, kept only with a row index, for its statistics; data: their varints)
  DevVec pres, vals, vals2, data;
  // this write call's batch, in the same form
  DevBuf b_bits, b_pres, b_vals, b_vals2, b_data, b_tmp;
  // nested: a Struct's / List's children's rows as a map (device/writer_nested.hip); a leaf's arrays gathered through its parent's
  DevBuf k_map, b_gath;
  // dictionary (orcgpu_writer_set_dictionary): the stripe being flushed -- whether the column is written DICTIONARY_V2, its
  // entries and their bytes, and the tables of device/writer_dict.hip (ids, entry lengths and bytes at these offsets of b_dict)
  bool dict = false;
  uint64_t dict_size = 0, dict_bytes = 0, o_dict_ids = 0, o_dict_len = 0, o_dict_data = 0;
  DevBuf b_dict;
  bool is_nest() const { return stream_kind >= 7; }
  int value_streams() const { return stream_kind == 7 ? 0 : (stream_kind == 8 || stream_kind < 4 ? 1 : (dict ? 3 : 2)); }
  bool has_bytes() const { return stream_kind == 4 || stream_kind == 6; }  // n_bytes / data count toward the estimate
  int elem2() const { return stream_kind == 5 ? 8 : 2; }
};

struct WrField {  // what ArrowWriter::write compares (batch.schema() == self.schema), at every level of the tree
  std::string format, name, metadata;
  int64_t flags = 0;
  bool dictionary = false;
  std::vector<WrField> kids;
  bool same(const WrField& o) const {
    if (format != o.format || name != o.name || metadata != o.metadata || (flags & 2) != (o.flags & 2) || dictionary != o.dictionary ||
        kids.size() != o.kids.size())
      return false;
    for (size_t i = 0; i < kids.size(); i++)
      if (!kids[i].same(o.kids[i])) return false;
    return true;
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

// Arrow C schema metadata: int32 count, then (int32 length, bytes) twice per pair -> its bytes
std::string wr_metadata(const char* m) {
  if (!m) return std::string();
  int32_t n;
  memcpy(&n, m, 4);
  size_t off = 4;
  for (int32_t i = 0; i < 2 * n; i++) {
    int32_t len;
    memcpy(&len, m + off, 4);
    off += 4 + (size_t)len;
  }
  return std::string(m, off);
}

// the column writer of an Arrow type (writer/stripe.rs:173-187, arrow_writer.rs:158-222); false: the reference's unimplemented!()
bool wr_column_of(const char* fmt, WrCol& c) {
  if (!fmt || !fmt[0]) return false;
  if (fmt[0] == 't' && fmt[1] == 's' && fmt[2] && fmt[3] == ':') {  // Timestamp(unit, tz): with a zone an instant
    switch (fmt[2]) {
      case 's': c.ups = 1; c.npu = 1000000000; break;
      case 'm': c.ups = 1000; c.npu = 1000000; break;
      case 'u': c.ups = 1000000; c.npu = 1000; break;
      case 'n': c.ups = 1000000000; c.npu = 1; break;
      default: return false;
    }
    c.elem = 8; c.stream_kind = 5; c.orc_kind = fmt[4] ? 18 : 9; c.encoding = 2;
    return true;
  }
  if (fmt[0] == 'd' && fmt[1] == ':') {  // Decimal128(p, s): "d:p,s" or "d:p,s,128"
    int p = 0, sc = 0, bits = 128, used = 0;
    const int got = sscanf(fmt + 2, "%d,%d%n", &p, &sc, &used);
    if (got != 2) return false;
    const char* rest = fmt + 2 + used;
    if (*rest) {
      int used2 = 0;
      if (sscanf(rest, ",%d%n", &bits, &used2) != 1 || rest[used2]) return false;
    }
    if (bits != 128 || p < 1 || p > 38 || sc < 0 || sc > p) return false;
    c.elem = 16; c.stream_kind = 6; c.orc_kind = 14; c.encoding = 2; c.precision = (uint32_t)p; c.scale = (uint32_t)sc;
    return true;
  }
  if (fmt[1]) return false;
  switch (fmt[0]) {
    case 'b': c.elem = 1; c.stream_kind = 3; c.orc_kind = 0; c.encoding = 0; return true;
    case 'c': c.elem = 1; c.stream_kind = 1; c.orc_kind = 1; c.encoding = 0; return true;
    case 's': c.elem = 2; c.stream_kind = 0; c.orc_kind = 2; c.encoding = 2; return true;
    case 'i': c.elem = 4; c.stream_kind = 0; c.orc_kind = 3; c.encoding = 2; return true;
    case 'l': c.elem = 8; c.stream_kind = 0; c.orc_kind = 4; c.encoding = 2; return true;
    case 'f': c.elem = 4; c.stream_kind = 2; c.orc_kind = 5; c.encoding = 0; return true;
    case 'g': c.elem = 8; c.stream_kind = 2; c.orc_kind = 6; c.encoding = 0; return true;
    case 'u': c.elem = 4; c.stream_kind = 4; c.orc_kind = 7; c.encoding = 2; c.is_string = true; return true;
    case 'U': c.elem = 8; c.stream_kind = 4; c.orc_kind = 7; c.encoding = 2; c.is_string = true; return true;
    case 'z': c.elem = 4; c.stream_kind = 4; c.orc_kind = 8; c.encoding = 2; c.is_string = true; return true;
    case 'Z': c.elem = 8; c.stream_kind = 4; c.orc_kind = 8; c.encoding = 2; c.is_string = true; return true;
    default: return false;
  }
}

bool wr_read_field(const ArrowSchema* c, WrField& f, int depth) {
  if (!c || !c->format || depth > 64 || c->n_children < 0 || (c->n_children && !c->children)) return false;
  f.format = c->format;
  f.name = c->name ? c->name : "";
  f.metadata = wr_metadata(c->metadata);
  f.flags = c->flags;
  f.dictionary = c->dictionary != nullptr;
  f.kids.resize((size_t)c->n_children);
  for (int64_t i = 0; i < c->n_children; i++)
    if (!wr_read_field(c->children[i], f.kids[(size_t)i], depth + 1)) return false;
  return true;
}

int wr_read_schema(orcgpu_ctx* ctx, const ArrowSchema* s, std::vector<WrField>& fields, std::string& md, int64_t& flags) {
  if (!s || !s->format || strcmp(s->format, "+s") != 0 || s->n_children < 0 || (s->n_children && !s->children)) {
    set_err(ctx, "writer: the schema must be an Arrow struct (format \"+s\") of its fields");
    return ORCGPU_INVALID_ARGUMENT;
  }
  fields.clear();
  fields.resize((size_t)s->n_children);
  for (int64_t i = 0; i < s->n_children; i++)
    if (!wr_read_field(s->children[i], fields[(size_t)i], 0)) return ORCGPU_INVALID_ARGUMENT;
  md = wr_metadata(s->metadata);
  flags = s->flags;
  return ORCGPU_OK;
}

int wr_unsupported(orcgpu_ctx* ctx, const WrField& f, const std::string& path, const char* why) {
  set_err(ctx, "writer: unsupported Arrow type '%s' of field '%s'%s (the reference: unimplemented!(\"unsupported datatype\"), writer/stripe.rs:186; beyond it: Timestamp, Decimal128, Struct, List, LargeList, Map)",
          f.format.c_str(), path.c_str(), why);
  return ORCGPU_UNSUPPORTED;
}

// a field and what is below it -> columns, preorder.  +s STRUCT, +l / +L LIST, +m MAP (its key and value: the entries struct
// gets no column); under_list: below a List or Map, where Decimal128 is not written
int wr_add_column(orcgpu_ctx* ctx, orcgpu_writer* w, const WrField& f, int parent, int child, const std::string& path, bool under_list) {
  const char* fmt = f.format.c_str();
  if (f.dictionary) return wr_unsupported(ctx, f, path, " (dictionary encoded)");
  WrCol c;
  const std::vector<WrField>* kids = nullptr;
  if (!strcmp(fmt, "+s")) {
    c.elem = 0; c.stream_kind = 7; c.orc_kind = 12; c.encoding = 0;
    kids = &f.kids;
  } else if (!strcmp(fmt, "+l") || !strcmp(fmt, "+L")) {
    if (f.kids.size() != 1) return ORCGPU_INVALID_ARGUMENT;
    c.elem = fmt[1] == 'l' ? 4 : 8; c.stream_kind = 8; c.orc_kind = 10; c.encoding = 2;
    kids = &f.kids;
    under_list = true;
  } else if (!strcmp(fmt, "+m")) {
    if (f.kids.size() != 1 || f.kids[0].format != "+s" || f.kids[0].kids.size() != 2) return ORCGPU_INVALID_ARGUMENT;
    c.elem = 4; c.stream_kind = 8; c.orc_kind = 11; c.encoding = 2;
    kids = &f.kids[0].kids;
    under_list = true;
  } else if (fmt[0] == '+') {  // FixedSizeList, ListView, Union, run-end encoded
    return wr_unsupported(ctx, f, path, "");
  } else {
    if (!wr_column_of(fmt, c)) return wr_unsupported(ctx, f, path, "");
    if (c.stream_kind == 6 && under_list) return wr_unsupported(ctx, f, path, " (Decimal128 below a List or Map)");
  }
  c.name = f.name;
  c.path = path;
  c.parent = parent;
  c.child = child;
  const int me = (int)w->cols.size();
  w->cols.push_back(std::move(c));
  if (parent >= 0) w->cols[(size_t)parent].kids.push_back(me);
  else w->root_kids.push_back(me);
  if (kids) {
    w->nested = true;
    for (size_t i = 0; i < kids->size(); i++) {
      const int rc = wr_add_column(ctx, w, (*kids)[i], me, (int)i, path + "." + (*kids)[i].name, under_list);
      if (rc) return rc;
    }
  }
  return ORCGPU_OK;
}

// the schema's columns and the options (the sink is the caller's)
int wr_prepare(orcgpu_ctx* ctx, const ArrowSchema* schema, const orcgpu_writer_opts* opts, orcgpu_writer* w) {
  w->ctx = ctx;
  int rc = wr_read_schema(ctx, schema, w->fields, w->root_metadata, w->root_flags);
  if (rc) return rc;
  for (size_t i = 0; i < w->fields.size(); i++) {
    rc = wr_add_column(ctx, w, w->fields[i], -1, (int)i, w->fields[i].name, false);
    if (rc) {
      if (rc == ORCGPU_INVALID_ARGUMENT) set_err(ctx, "writer: field '%s' is not a well-formed Arrow type", w->fields[i].name.c_str());
      return rc;
    }
  }
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

// an upper bound of an encoded stream of n values (RLE v2: a run of one value is 2 header bytes + the value, a DELTA of three
// values a header, two varints of up to 10 bytes and the packed delta, PATCHED_BASE adds its patch list; byte RLE: a header byte
// per value and the value)
inline uint64_t wr_stream_bound(int kind, int int_bytes, uint64_t n) { return kind == 1 ? 2 * n + 2 : (uint64_t)(3 * int_bytes + 12) * n + 64; }

// DevBuf::ensure waits for the device when it grows (hipFree): counted
bool wr_ensure(orcgpu_writer* w, DevBuf& b, uint64_t n) {
  if (n > b.cap) w->round_trips++;
  return b.ensure(n);
}
bool wr_reserve(orcgpu_writer* w, DevVec& v, uint64_t n, uint64_t used) {
  if (n > v.cap && v.p) w->round_trips++;
  return v.reserve(n, used, w->ctx->stream);
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
int wr_rle_stream(orcgpu_writer* w, int kind, const void* d_values, uint64_t n, int int_bytes, int is_signed, uint64_t* at, uint64_t li,
                  const WrIxPos* ip = nullptr) {
  orcgpu_ctx* ctx = w->ctx;
  uint64_t* d_lens = (uint64_t*)w->lens.p;
  if (!n) {
    WR_TRY(hipMemsetAsync(d_lens + li, 0, 8, ctx->stream));
    WR_TRY(wr_ix_pos(ctx, ip, nullptr));
    return ORCGPU_OK;
  }
  EncJob J;
  J.kind = kind;
  J.int_bytes = int_bytes;
  J.is_signed = is_signed;
  J.n = n;
  J.values = d_values;
  J.deferred = true;
  J.syncs = &w->round_trips;
  int rc = enc_plan(ctx, J);
  if (rc) return rc;
  const uint64_t room = wr_stream_bound(kind, int_bytes, n);
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
  return wr_rle_stream(w, 1, rev, nb, 1, 0, at, li, ip);
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


// ---- row index: statistics on the host ------------------------------------------------------------------------------------
// a group's record as the device wrote it; side: the string copies
WrStat wr_stat_of(const WrCol& c, const IxRec& r, const uint8_t* side) {
  WrStat s;
  s.count = r.count;
  s.has_null = r.has_null != 0;
  if (!r.count) return s;
  switch (c.stream_kind) {
    case 0: case 1:
      s.imin = r.imin;
      s.imax = r.imax;
      s.isum = (__int128)(((unsigned __int128)(uint64_t)r.sum_hi << 64) | r.sum_lo);
      break;
    case 2: s.dmin = r.dmin; s.dmax = r.dmax; s.dsum = r.dsum; s.dsum_lo = r.dsum_lo; s.dbig = r.dbig; s.dbig_lo = r.dbig_lo; s.has_nan = r.has_nan != 0; break;
    case 3: s.trues = r.trues; break;
    case 5: s.imin = r.imin; s.imax = r.imax; s.nmin = (uint32_t)r.sum_lo; s.nmax = (uint32_t)r.sum_hi; break;
    case 6:
      s.qmin = (__int128)(((unsigned __int128)(uint64_t)r.imax << 64) | (uint64_t)r.imin);
      s.qmax = (__int128)(((unsigned __int128)r.smax_at << 64) | r.smin_at);
      s.qsum[0] = r.sum_lo, s.qsum[1] = (uint64_t)r.sum_hi, s.qsum[2] = r.trues, s.qsum[3] = (uint64_t)((int64_t)r.trues >> 63);
      break;
    default:
      s.bytes = r.bytes;
      if (c.orc_kind == 7) {
        const uint32_t a = std::min(r.smin_len, IX_STR_KEEP), b = std::min(r.smax_len, IX_STR_KEEP);
        s.smin.assign((const char*)side + r.side, a);
        s.smax.assign((const char*)side + r.side + a, b);
        s.smin_len = r.smin_len;
        s.smax_len = r.smax_len;
      }
      break;
  }
  return s;
}

// byte order of two strings known by their first IX_STR_KEEP bytes (two cut ones with equal prefixes have the same bound)
int wr_str_cmp(const std::string& a, uint64_t la, const std::string& b, uint64_t lb) {
  const int c = memcmp(a.data(), b.data(), std::min(a.size(), b.size()));
  if (c) return c;
  if (a.size() == b.size()) return a.size() == la && b.size() == lb ? (la < lb ? -1 : (la > lb ? 1 : 0)) : 0;
  return a.size() < b.size() ? -1 : 1;
}

void wr_dd_merge(double& hi, double& lo, double h2, double l2) {
#pragma clang fp contract(off)
  if (!std::isfinite(hi) || !std::isfinite(h2)) {
    hi += h2;
    lo = 0;
    return;
  }
  const double s = hi + h2, bb = s - hi;
  double e = (hi - (s - bb)) + (h2 - bb);
  e += lo + l2;
  hi = s + e;
  lo = e - (hi - s);
}

// b's rows follow a's (minimum / maximum: the first of equal values stays)
void wr_stat_merge(WrStat& a, const WrStat& b) {
  a.has_null |= b.has_null;
  a.has_nan |= b.has_nan;
  if (b.count) {
    const bool first = a.count == 0;
    // (Timestamp: the nanoseconds go with their seconds; every other column leaves them 0)
    if (first || b.imin < a.imin || (b.imin == a.imin && b.nmin < a.nmin)) a.imin = b.imin, a.nmin = b.nmin;
    if (first || b.imax > a.imax || (b.imax == a.imax && b.nmax > a.nmax)) a.imax = b.imax, a.nmax = b.nmax;
    if (first || b.qmin < a.qmin) a.qmin = b.qmin;
    if (first || b.qmax > a.qmax) a.qmax = b.qmax;
    unsigned carry = 0;
    for (int i = 0; i < 4; i++) {
      const unsigned __int128 t = (unsigned __int128)a.qsum[i] + b.qsum[i] + carry;
      a.qsum[i] = (uint64_t)t;
      carry = (unsigned)(t >> 64);
    }
    if (first || b.dmin < a.dmin) a.dmin = b.dmin;
    if (first || b.dmax > a.dmax) a.dmax = b.dmax;
    if (first || wr_str_cmp(b.smin, b.smin_len, a.smin, a.smin_len) < 0) a.smin = b.smin, a.smin_len = b.smin_len;
    if (first || wr_str_cmp(b.smax, b.smax_len, a.smax, a.smax_len) > 0) a.smax = b.smax, a.smax_len = b.smax_len;
    a.isum += b.isum;
    if (first) a.dsum = b.dsum, a.dsum_lo = b.dsum_lo, a.dbig = b.dbig, a.dbig_lo = b.dbig_lo;
    else wr_dd_merge(a.dsum, a.dsum_lo, b.dsum, b.dsum_lo), wr_dd_merge(a.dbig, a.dbig_lo, b.dbig, b.dbig_lo);
    a.bytes += b.bytes;
    a.trues += b.trues;
  }
  a.count += b.count;
}

// StringStatisticsImpl's bounds of a value longer than 1024 bytes: the longest prefix of at most 1024 bytes that ends at a
// character boundary; for the upper bound its last character's code point incremented
std::string wr_lower_bound(const std::string& s) {
  size_t cut = 1024;
  while (cut > 0 && ((uint8_t)s[cut] & 0xc0) == 0x80) cut--;
  return s.substr(0, cut);
}
// (trailing U+10FFFF have no successor: they are dropped first; false when nothing is left, and no bound is an upper bound)
bool wr_upper_bound(const std::string& s, std::string& out) {
  std::string p = wr_lower_bound(s);
  uint32_t cp = 0;
  size_t k = 0;
  for (;;) {
    if (p.empty()) return false;
    k = p.size() - 1;
    while (k > 0 && ((uint8_t)p[k] & 0xc0) == 0x80) k--;
    const uint8_t h = (uint8_t)p[k];
    const size_t n = p.size() - k;
    cp = n == 1 ? h : (h & (0xffu >> (n + 1)));
    for (size_t i = 1; i < n; i++) cp = (cp << 6) | ((uint8_t)p[k + i] & 0x3f);
    if (cp < 0x10ffff) break;
    p.resize(k);
  }
  cp++;
  if (cp >= 0xd800 && cp < 0xe000) cp = 0xe000;
  std::string e;
  if (cp < 0x80) e += (char)cp;
  else if (cp < 0x800) e += (char)(0xc0 | (cp >> 6)), e += (char)(0x80 | (cp & 0x3f));
  else if (cp < 0x10000) e += (char)(0xe0 | (cp >> 12)), e += (char)(0x80 | ((cp >> 6) & 0x3f)), e += (char)(0x80 | (cp & 0x3f));
  else
    e += (char)(0xf0 | (cp >> 18)), e += (char)(0x80 | ((cp >> 12) & 0x3f)), e += (char)(0x80 | ((cp >> 6) & 0x3f)), e += (char)(0x80 | (cp & 0x3f));
  out = p.substr(0, k) + e;
  return true;
}

// a float range's sum: the two double-doubles added, with the big one's scale; infinite when the exact sum is beyond f64 (an
// infinite input: the big one is infinite or NaN, and that is the sum)
double wr_float_sum(const WrStat& s) {
#pragma clang fp contract(off)
  if (!std::isfinite(s.dbig)) return s.dbig;
  if (s.dbig == 0 && s.dbig_lo == 0) return s.dsum + s.dsum_lo;
  double hi = s.dbig, lo = s.dbig_lo;
  wr_dd_merge(hi, lo, std::ldexp(s.dsum, -64), std::ldexp(s.dsum_lo, -64));
  return std::ldexp(hi + lo, 64);
}

// a decimal at `scale` in minimal form: no exponent, trailing fractional zeros and a bare point removed, "0" for zero
std::string wr_decimal_string(__int128 v, uint32_t scale) {
  const bool neg = v < 0;
  unsigned __int128 m = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
  std::string d;
  while (m) d.insert(d.begin(), (char)('0' + (int)(m % 10))), m /= 10;
  if (d.size() <= scale) d.insert(0, scale + 1 - d.size(), '0');
  if (scale) {
    d.insert(d.size() - scale, ".");
    while (d.back() == '0') d.pop_back();
    if (d.back() == '.') d.pop_back();
  }
  if (d.empty()) d = "0";
  return neg ? "-" + d : d;
}

// ColumnStatistics (c: nullptr for the root struct, whose values are its rows)
PbOut wr_stat_msg(const WrCol* c, const WrStat& s) {
  PbOut m;
  m.u64(1, s.count);
  if (c && s.count) {
    PbOut t;
    switch (c->stream_kind) {
      case 0: case 1:
        t.sint(1, s.imin);
        t.sint(2, s.imax);
        if (s.isum >= (__int128)INT64_MIN && s.isum <= (__int128)INT64_MAX) t.sint(3, (int64_t)s.isum);
        m.msg(2, t);
        break;
      case 2:
        if (s.has_nan) break;  // (no DoubleStatistics: a reader would take an absent bound for 0)
        t.f64(1, s.dmin);
        t.f64(2, s.dmax);
        t.f64(3, wr_float_sum(s));
        m.msg(3, t);
        break;
      case 3:
        t.packed(1, {s.trues});
        m.msg(5, t);
        break;
      case 5: {  // TimestampStatistics: floor milliseconds (the writer's zone is UTC: the legacy fields hold the same), and the
                 // nanoseconds within the millisecond plus one; none when a bound's milliseconds leave i64
        const __int128 lo = (__int128)s.imin * 1000 + s.nmin / 1000000, hi = (__int128)s.imax * 1000 + s.nmax / 1000000;
        if (lo < (__int128)INT64_MIN || hi > (__int128)INT64_MAX) break;
        t.sint(1, (int64_t)lo);
        t.sint(2, (int64_t)hi);
        t.sint(3, (int64_t)lo);
        t.sint(4, (int64_t)hi);
        t.u64(5, s.nmin % 1000000 + 1);
        t.u64(6, s.nmax % 1000000 + 1);
        m.msg(9, t);
        break;
      }
      case 6: {  // DecimalStatistics: the sum when |sum| < 10^38
        const std::string a = wr_decimal_string(s.qmin, c->scale), b = wr_decimal_string(s.qmax, c->scale);
        t.bytes(1, a.data(), a.size());
        t.bytes(2, b.data(), b.size());
        const uint64_t ext = (uint64_t)((int64_t)s.qsum[1] >> 63);
        if (s.qsum[2] == ext && s.qsum[3] == ext) {
          const __int128 sum = (__int128)(((unsigned __int128)s.qsum[1] << 64) | s.qsum[0]);
          __int128 lim = 1;
          for (int i = 0; i < 38; i++) lim *= 10;
          if (sum < lim && sum > -lim) {
            const std::string z = wr_decimal_string(sum, c->scale);
            t.bytes(3, z.data(), z.size());
          }
        }
        m.msg(6, t);
        break;
      }
      default:
        if (c->orc_kind == 8) {
          t.sint(1, (int64_t)s.bytes);
          m.msg(8, t);
          break;
        }
        std::string ub;
        if (s.smax_len > 1024 && !wr_upper_bound(s.smax, ub)) break;  // (no upper bound: no StringStatistics, nothing is pruned)
        if (s.smin_len <= 1024) t.bytes(1, s.smin.data(), s.smin.size());
        if (s.smax_len <= 1024) t.bytes(2, s.smax.data(), s.smax.size());
        t.sint(3, (int64_t)s.bytes);
        if (s.smin_len > 1024) {
          const std::string lb = wr_lower_bound(s.smin);
          t.bytes(4, lb.data(), lb.size());
        }
        if (s.smax_len > 1024) t.bytes(5, ub.data(), ub.size());
        m.msg(4, t);
        break;
    }
  }
  m.u64(10, s.has_null ? 1 : 0);
  return m;
}

// the positions of a column's streams for one group, PRESENT, DATA, LENGTH (form: 1 bytes, 2 run-length, 3 bits over byte runs)
void wr_positions(const uint64_t* pos, uint64_t G, uint64_t g, bool comp, const std::vector<std::pair<uint64_t, int>>& streams, std::vector<uint64_t>& out) {
  for (auto& st : streams) {
    const uint64_t* p = pos + (st.first * G + g) * 4;
    out.push_back(p[0]);
    if (comp) out.push_back(p[1]);
    if (st.second >= 2) out.push_back(p[2]);
    if (st.second == 3) out.push_back(p[3]);
  }
}

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
    if (w->dict_threshold > 0 && c.orc_kind == 7 && c.n_valid) dc.push_back(ci);
  }
  if (dc.empty()) return ORCGPU_OK;
  const uint64_t K = dc.size();
  if (!wr_ensure(w, w->dict_res, (2 * K + 1) * 8 + kAlign)) return ORCGPU_HIP_ERROR;
  uint64_t* d_res = (uint64_t*)w->dict_res.p;  // [column] entries, bytes; then `bad`
  uint32_t* d_bad = (uint32_t*)(d_res + 2 * K);
  WR_TRY(hipMemsetAsync(d_bad, 0, 8, st));
  for (uint64_t k = 0; k < K; k++) {
    WrCol& c = w->cols[dc[k]];
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
    c.o_dict_ids = T.take(n * (uint64_t)c.elem);
    c.o_dict_len = T.take(n * (uint64_t)c.elem);
    c.o_dict_data = T.take(align_up(c.n_bytes, 16) + 16);
    if (!wr_ensure(w, c.b_dict, T.off + kAlign)) {
      set_err(ctx, "writer: out of device memory (%llu bytes of dictionary tables)", (unsigned long long)T.off);
      return ORCGPU_HIP_ERROR;
    }
    uint8_t* t = c.b_dict.p;
    uint32_t *len32 = (uint32_t*)(t + o_len32), *rep = (uint32_t*)(t + o_table), *low = rep + slots, *slot_of = (uint32_t*)(t + o_slot),
             *flag = (uint32_t*)(t + o_flag), *flen = (uint32_t*)(t + o_flen), *erow = (uint32_t*)(t + o_erow);
    uint64_t *offs = (uint64_t*)(t + o_offs), *sums = (uint64_t*)(t + o_sums), *first = (uint64_t*)(t + o_first), *foff = (uint64_t*)(t + o_foff),
             *tot_d = (uint64_t*)(t + o_d), *tot_D = (uint64_t*)(t + o_D), *eoff = (uint64_t*)(t + o_eoff);
    WR_TRY(launch(wd_len32_kernel, n, false, 256, st, (const void*)c.vals.p, c.elem, n, len32));
    int rc = enc_scan(ctx, st, len32, n, sums, (uint64_t*)(t + o_tot), offs);
    if (rc) return rc;
    WR_TRY(hipMemsetAsync(rep, 0xff, slots * 8, st));
    WR_TRY(launch(wd_insert_kernel, n, false, 256, st, (const uint8_t*)c.data.p, (const uint64_t*)offs, (const uint32_t*)len32, (uint32_t)n, rep, low,
                  (uint32_t)(slots - 1), w->dict_hash_mask, slot_of, d_bad));
    WR_TRY(launch(wd_flag_kernel, n, false, 256, st, (const uint32_t*)slot_of, (const uint32_t*)low, (const uint32_t*)len32, (uint32_t)n, flag, flen));
    rc = enc_scan(ctx, st, flag, n, sums, tot_d, first);
    if (rc) return rc;
    rc = enc_scan(ctx, st, flen, n, sums, tot_D, foff);
    if (rc) return rc;
    WR_TRY(launch(wd_ids_kernel, n, false, 256, st, (const uint32_t*)slot_of, (const uint32_t*)low, (const uint32_t*)flag, (const uint64_t*)first,
                  (const uint64_t*)foff, (const uint32_t*)len32, (uint32_t)n, c.elem, (void*)(t + c.o_dict_ids), (void*)(t + c.o_dict_len), erow, eoff, d_bad));
    WR_TRY(launch(wd_gather_kernel, (c.n_bytes + 15) / 16, false, 256, st, (const uint8_t*)c.data.p, (const uint64_t*)offs, (const uint32_t*)erow,
                  (const uint64_t*)eoff, (const uint64_t*)tot_d, (const uint64_t*)tot_D, (uint4*)(t + c.o_dict_data)));
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
    const uint64_t d = res[2 * k];
    if (d > c.n_valid || res[2 * k + 1] > c.n_bytes) return ORCGPU_UNEXPECTED;
    if ((double)d <= w->dict_threshold * (double)c.n_valid) {
      c.dict = true;
      c.dict_size = d;
      c.dict_bytes = res[2 * k + 1];
    }
  }
  return ORCGPU_OK;
}

// StripeWriter::finish_stripe (writer/stripe.rs:109-165) + ArrowWriter::flush_stripe.  Every stream of every column is enqueued
// without a host wait, each into a slot of its bound; then two waits, whatever the column count: the streams' lengths come back,
// and the streams, moved back to back on the device, reach the host in one copy.
int wr_flush(orcgpu_writer* w) {
  orcgpu_ctx* ctx = w->ctx;
  const uint64_t trips0 = w->round_trips;
  struct St {
    int kind;
    uint32_t column;
    uint64_t slot;
  };
  std::vector<St> streams;
  int rc = wr_dictionaries(w);
  if (rc) return rc;
  // room: the lengths, the bitmaps of the Boolean / PRESENT streams
  uint64_t n_streams = 0, bits_room = 0;
  for (auto& c : w->cols) {
    n_streams += c.value_streams() + c.present;
    if (c.stream_kind == 3) bits_room += align_up(2 * ((c.n_valid + 7) / 8) + 16);
    if (c.present) bits_room += align_up(2 * ((c.rows + 7) / 8) + 16);
  }
  if (!wr_ensure(w, w->lens, n_streams * 8 + kAlign) || !wr_ensure(w, w->bits, bits_room + kAlign)) return ORCGPU_HIP_ERROR;
  w->bits_at = 0;
  std::vector<uint64_t> known(n_streams, ~0ull);
  uint64_t at = 0;
  // row index: the groups' statistics, enqueued ahead of the streams (jobs: column * G + group)
  const size_t nc = w->cols.size();
  const bool indexed = w->stride > 0;
  const uint64_t S = w->stride, G = indexed ? (w->rows + S - 1) / S : 0, NJ = nc * G;
  uint64_t o_cols = 0, o_cnt = 0, o_vscan = 0, o_blen = 0, o_bscan = 0, o_slen = 0, o_soff = 0, o_recs = 0, o_pos = 0, o_side = 0, ix_span = 0;
  std::vector<std::vector<std::pair<uint64_t, int>>> ix_streams(nc);  // a column's streams (index, position form), PRESENT, DATA, LENGTH
  if (NJ) {
    if (NJ >= 0x7fffffffull) {
      set_err(ctx, "writer: %llu row groups in one stripe (fewer than 2^31)", (unsigned long long)NJ);
      return ORCGPU_INVALID_ARGUMENT;
    }
    uint64_t side_bound = 0;
    for (auto& c : w->cols)
      if (c.orc_kind == 7) side_bound += std::min<uint64_t>(2ull * IX_STR_KEEP * G, 2 * c.n_bytes);
    Bump X;
    o_cols = X.take(nc * sizeof(IxCol));
    o_cnt = X.take(NJ * 8);
    o_vscan = X.take((NJ + 1) * 8);
    o_blen = X.take(NJ * 8);
    o_bscan = X.take((NJ + 1) * 8);
    o_slen = X.take(NJ * 8);
    o_soff = X.take((NJ + 1) * 8);
    o_recs = X.take(NJ * sizeof(IxRec));  // (from here on: brought back)
    o_pos = X.take(n_streams * G * 32);
    o_side = X.take(side_bound);
    ix_span = X.off - o_recs;
    if (!wr_reserve(w, w->ix, X.off + kAlign, 0)) {
      set_err(ctx, "writer: out of device memory (%llu bytes of row index)", (unsigned long long)X.off);
      return ORCGPU_HIP_ERROR;
    }
    if (ix_span > w->ix_pinned_cap) {
      if (w->ix_pinned) {
        (void)hipHostFree(w->ix_pinned);
        w->round_trips++;  // (hipHostFree waits for the device)
      }
      w->ix_pinned = nullptr;
      w->ix_pinned_cap = 0;
      WR_TRY(hipHostMalloc((void**)&w->ix_pinned, ix_span + ix_span / 2, 0));
      w->ix_pinned_cap = ix_span + ix_span / 2;
    }
    uint8_t* x = w->ix.p;
    IxCol* d_cols = (IxCol*)(x + o_cols);
    for (uint32_t i0 = 0; i0 < nc; i0 += IX_COLS_PER_ARG) {
      IxColArgs a{};
      a.at = i0;
      a.n = std::min<uint32_t>(IX_COLS_PER_ARG, (uint32_t)nc - i0);
      for (uint32_t i = 0; i < a.n; i++) {
        const WrCol& c = w->cols[i0 + i];
        a.c[i] = IxCol{c.pres.p, c.vals.p, c.stream_kind == 5 ? c.vals2.p : c.data.p, c.stream_kind, c.elem, c.orc_kind == 7, 0};
      }
      WR_TRY(launch(ix_put_cols_kernel, (uint64_t)1, true, 64, ctx->stream, a, d_cols));
    }
    uint64_t *d_cnt = (uint64_t*)(x + o_cnt), *d_vscan = (uint64_t*)(x + o_vscan), *d_blen = (uint64_t*)(x + o_blen), *d_bscan = (uint64_t*)(x + o_bscan),
             *d_slen = (uint64_t*)(x + o_slen), *d_soff = (uint64_t*)(x + o_soff);
    IxRec* d_recs = (IxRec*)(x + o_recs);
    const IxCol* cc = d_cols;
    WR_TRY(launch(ix_count_kernel, NJ, true, 256, ctx->stream, cc, w->rows, S, G, d_cnt));
    WR_TRY(launch(ix_scan_kernel, (uint64_t)1, true, 1024, ctx->stream, (const uint64_t*)d_cnt, NJ, d_vscan));
    WR_TRY(launch(ix_bytes_kernel, NJ, true, 256, ctx->stream, cc, G, (const uint64_t*)d_cnt, (const uint64_t*)d_vscan, d_blen));
    WR_TRY(launch(ix_scan_kernel, (uint64_t)1, true, 1024, ctx->stream, (const uint64_t*)d_blen, NJ, d_bscan));
    WR_TRY(launch(ix_stats_kernel, NJ, true, 256, ctx->stream, cc, w->rows, S, G, (const uint64_t*)d_cnt, (const uint64_t*)d_vscan, (const uint64_t*)d_bscan,
                  d_recs, d_slen));
    WR_TRY(launch(ix_scan_kernel, (uint64_t)1, true, 1024, ctx->stream, (const uint64_t*)d_slen, NJ, d_soff));
    WR_TRY(launch(ix_side_kernel, NJ, true, 256, ctx->stream, cc, G, (const uint64_t*)d_soff, d_recs, x + o_side));
  }
  // a stream's positions: ix_pos_kernel's mode, the values (bits) of the stream
  auto ixp = [&](int mode, size_t ci, uint64_t n, uint64_t li, int form) -> WrIxPos {
    if (!NJ) return WrIxPos{mode, 0, 0, 0, nullptr, nullptr, 0, nullptr};
    ix_streams[ci].push_back({li, form});
    uint8_t* x = w->ix.p;
    return WrIxPos{mode, G, S, n, (const uint64_t*)(x + o_vscan) + ci * G, (const uint64_t*)(x + o_bscan) + ci * G, w->cols[ci].elem,
                   (uint64_t*)(x + o_pos) + li * G * 4};
  };
  for (size_t ci = 0; ci < w->cols.size(); ci++) {
    WrCol& c = w->cols[ci];
    const uint32_t column = (uint32_t)ci + 1;
    // (the positions list PRESENT first: its stream index is known before it is written)
    const uint64_t li_present = streams.size() + c.value_streams();
    if (c.present) ixp(0, ci, c.rows, li_present, 3);
    uint64_t li = streams.size();
    if (c.value_streams()) streams.push_back(St{c.stream_kind == 8 ? 2 : 1, column, at});
    WrIxPos ip;
    if (c.dict) {
      // DICTIONARY_V2: DATA the rows' ids (positions as an integer column's), LENGTH the entries' lengths, DICTIONARY_DATA their
      // bytes; the row index holds nothing for the last two
      ip = ixp(1, ci, c.n_valid, li, 2);
      rc = wr_rle_stream(w, 0, c.b_dict.p + c.o_dict_ids, c.n_valid, c.elem, 0, &at, li, &ip);
      if (rc) return rc;
      li = streams.size();
      streams.push_back(St{2, column, at});
      rc = wr_rle_stream(w, 0, c.b_dict.p + c.o_dict_len, c.dict_size, c.elem, 0, &at, li);
      if (rc) return rc;
      li = streams.size();
      streams.push_back(St{3, column, at});
      rc = wr_copy_stream(w, c.b_dict.p + c.o_dict_data, c.dict_bytes, &at, li, known);
      if (rc) return rc;
      if (NJ) WR_TRY(hipMemsetAsync(w->ix.p + o_pos + (li - 1) * G * 32, 0, 2 * G * 32, ctx->stream));
    } else switch (c.stream_kind) {
      case 7: break;  // a Struct: PRESENT alone
      case 8: rc = wr_rle_stream(w, 0, c.vals.p, c.n_valid, c.elem, 0, &at, li); break;  // LENGTH
      case 0: ip = ixp(1, ci, c.n_valid, li, 2); rc = wr_rle_stream(w, 0, c.vals.p, c.n_valid, c.elem, 1, &at, li, &ip); break;
      case 1: ip = ixp(2, ci, c.n_valid, li, 2); rc = wr_rle_stream(w, 1, c.vals.p, c.n_valid, 1, 0, &at, li, &ip); break;
      case 2:
        ip = ixp(4, ci, c.n_valid, li, 1);
        rc = wr_copy_stream(w, c.vals.p, c.n_valid * (uint64_t)c.elem, &at, li, known);
        if (!rc && wr_ix_pos(ctx, &ip, nullptr) != hipSuccess) rc = ORCGPU_HIP_ERROR;
        break;
      case 3: ip = ixp(3, ci, c.n_valid, li, 3); rc = wr_bool_stream(w, c.vals.p, c.n_valid, &at, li, &ip); break;
      case 5: ip = ixp(1, ci, c.n_valid, li, 2); rc = wr_rle_stream(w, 0, c.vals.p, c.n_valid, 8, 1, &at, li, &ip); break;
      default:  // strings' bytes, decimals' varints
        ip = ixp(5, ci, c.n_valid, li, 1);
        rc = wr_copy_stream(w, c.data.p, c.n_bytes, &at, li, known);
        if (!rc && wr_ix_pos(ctx, &ip, nullptr) != hipSuccess) rc = ORCGPU_HIP_ERROR;
        break;
    }
    if (rc) return rc;
    if (c.stream_kind == 4 && !c.dict) {
      li = streams.size();
      streams.push_back(St{2, column, at});
      ip = ixp(1, ci, c.n_valid, li, 2);
      rc = wr_rle_stream(w, 0, c.vals.p, c.n_valid, c.elem, 0, &at, li, &ip);
      if (rc) return rc;
    } else if (c.stream_kind == 5 || c.stream_kind == 6) {  // SECONDARY: the nanosecond codes (unsigned); the scale (signed)
      li = streams.size();
      streams.push_back(St{5, column, at});
      ip = ixp(1, ci, c.n_valid, li, 2);
      rc = wr_rle_stream(w, 0, c.vals2.p, c.n_valid, c.elem2(), c.stream_kind == 6, &at, li, &ip);
      if (rc) return rc;
    }
    if (c.present) {
      li = streams.size();
      streams.push_back(St{0, column, at});
      if (NJ) {
        uint8_t* x = w->ix.p;
        ip = WrIxPos{0, G, S, c.rows, (const uint64_t*)(x + o_vscan) + ci * G, nullptr, 0, (uint64_t*)(x + o_pos) + li * G * 4};
      }
      rc = wr_bool_stream(w, c.pres.p, c.rows, &at, li, NJ ? &ip : nullptr);
      if (rc) return rc;
    }
  }
  // compression: every stream from its slot into its slot of zout, in one launch set; the lengths in w->lens become the chunks'
  const bool comp = w->comp != ORCGPU_COMP_NONE;
  std::vector<uint64_t> zslot(n_streams, 0);
  if (comp && n_streams) {
    std::vector<LzcStream> jobs(n_streams);
    std::vector<uint64_t> rooms(n_streams);
    uint64_t zat = 0;
    for (uint64_t i = 0; i < n_streams; i++) {
      rooms[i] = (i + 1 < n_streams ? streams[i + 1].slot : at) - streams[i].slot;
      zslot[i] = zat;
      jobs[i] = LzcStream{streams[i].slot, zat, known[i]};
      zat += align_up(lzc_room(rooms[i], w->comp_block));
    }
    if (!wr_reserve(w, w->zout, zat + kAlign, 0)) {
      set_err(ctx, "writer: out of device memory (%llu bytes of compressed stripe)", (unsigned long long)zat);
      return ORCGPU_HIP_ERROR;
    }
    const LzcPlan* d_plan = nullptr;
    const uint64_t* d_chunk_off = nullptr;
    rc = lzc_enqueue(ctx, lzc_codec(w->comp), w->comp_block, w->slots.p, w->zout.p, jobs, rooms, (uint64_t*)w->lens.p, &w->round_trips, &d_plan, &d_chunk_off);
    if (rc) return rc;
    if (NJ)
      WR_TRY(launch(ix_map_kernel, n_streams * G, false, 256, ctx->stream, n_streams * G, G, w->comp_block, d_plan, d_chunk_off, (uint64_t*)(w->ix.p + o_pos)));
  }
  // the row index comes back with the lengths
  if (NJ) WR_TRY(hipMemcpyAsync(w->ix_pinned, w->ix.p + o_recs, ix_span, hipMemcpyDeviceToHost, ctx->stream));
  std::vector<uint64_t> lens(n_streams, 0);
  if (n_streams) WR_TRY(hipMemcpyAsync(lens.data(), w->lens.p, n_streams * 8, hipMemcpyDeviceToHost, ctx->stream));
  rc = wr_sync(w);
  if (rc) return rc;
  // ROW_INDEX streams (column 0 first) and the stripe's statistics
  std::vector<std::vector<uint8_t>> index;
  if (indexed) {
    const IxRec* recs = (const IxRec*)w->ix_pinned;
    const uint64_t* pos = (const uint64_t*)(w->ix_pinned + (o_pos - o_recs));
    const uint8_t* side = w->ix_pinned + (o_side - o_recs);
    std::vector<WrStat> stripe(nc + 1);
    stripe[0].count = w->rows;
    PbOut root;
    for (uint64_t g = 0; g < G; g++) {
      WrStat s;
      s.count = std::min(S, w->rows - g * S);
      PbOut e;
      e.msg(2, wr_stat_msg(nullptr, s));
      root.msg(1, e);
    }
    index.push_back(root.b);
    for (size_t ci = 0; ci < nc; ci++) {
      PbOut ri;
      std::vector<uint64_t> p;
      for (uint64_t g = 0; g < G; g++) {
        const WrStat s = wr_stat_of(w->cols[ci], recs[ci * G + g], side);
        wr_stat_merge(stripe[ci + 1], s);
        p.clear();
        wr_positions(pos, G, g, comp, ix_streams[ci], p);
        PbOut e;
        e.packed(1, p);
        e.msg(2, wr_stat_msg(&w->cols[ci], s));
        ri.msg(1, e);
      }
      index.push_back(ri.b);
    }
    if (comp)
      for (auto& b : index) b = lzc_original_chunks(b, w->comp_block);
    w->stripe_stats.push_back(std::move(stripe));
  }
  uint64_t total = 0;
  for (uint64_t i = 0; i < n_streams; i++) {
    if (known[i] != ~0ull && !comp) lens[i] = known[i];
    total += lens[i];
  }
  // back to back in the stripe's stream order, then one copy to pinned memory
  if (!wr_reserve(w, w->out, total + kAlign, 0)) return ORCGPU_HIP_ERROR;
  uint64_t pos = 0;
  for (uint64_t i = 0; i < n_streams; i++) {
    const uint8_t* src = comp ? w->zout.p + zslot[i] : w->slots.p + streams[i].slot;
    if (lens[i]) WR_TRY(hipMemcpyAsync(w->out.p + pos, src, lens[i], hipMemcpyDeviceToDevice, ctx->stream));
    pos += lens[i];
  }
  if (total > w->pinned_cap) {
    if (w->pinned) (void)hipHostFree(w->pinned);
    w->pinned = nullptr;
    w->pinned_cap = 0;
    w->round_trips++;  // (hipHostMalloc / hipHostFree wait for the device)
    WR_TRY(hipHostMalloc((void**)&w->pinned, total + total / 2, 0));
    w->pinned_cap = total + total / 2;
  }
  if (total) WR_TRY(hipMemcpyAsync(w->pinned, w->out.p, total, hipMemcpyDeviceToHost, ctx->stream));
  rc = wr_sync(w);
  if (rc) return rc;
  PbOut footer;
  uint64_t index_length = 0;
  for (size_t ci = 0; ci < index.size(); ci++) {
    PbOut m;
    m.u64(1, 6);  // ROW_INDEX
    m.u64(2, ci);
    m.u64(3, index[ci].size());
    footer.msg(1, m);
    index_length += index[ci].size();
  }
  for (uint64_t i = 0; i < n_streams; i++) {
    PbOut m;
    m.u64(1, (uint64_t)streams[i].kind);
    m.u64(2, streams[i].column);
    m.u64(3, lens[i]);
    footer.msg(1, m);
  }
  for (size_t ci = 0; ci <= w->cols.size(); ci++) {
    PbOut m;
    m.u64(1, ci ? (w->cols[ci - 1].dict ? 3u : (uint64_t)w->cols[ci - 1].encoding) : 0u);
    if (ci && w->cols[ci - 1].dict) m.u64(2, w->cols[ci - 1].dict_size);
    footer.msg(2, m);
  }
  for (auto& c : w->cols)
    if (c.stream_kind == 5) {  // (without it Apache ORC reads TIMESTAMP columns in the reading host's zone)
      footer.bytes(3, "UTC", 3);
      break;
    }
  if (comp) footer.b = lzc_original_chunks(footer.b, w->comp_block);
  const uint64_t start = w->written;
  for (auto& b : index) {
    rc = wr_sink(w, b.data(), b.size());
    if (rc) return rc;
  }
  rc = wr_sink(w, w->pinned, total);
  if (rc) return rc;
  rc = wr_sink(w, footer.b.data(), footer.b.size());
  if (rc) return rc;
  w->stripes.push_back(WrStripe{start, total, footer.b.size(), w->rows, index_length});
  w->rows = 0;
  for (auto& c : w->cols) {
    if (c.orc_kind == 7) (c.dict ? w->n_dictionary : w->n_direct)++;
    c.dict = false;
  }
  for (auto& c : w->cols) c.rows = c.n_valid = c.n_bytes = 0;
  w->base_rle = 0;
  for (auto& c : w->cols) c.base_valid = 0;
  w->stripe_round_trips += w->round_trips - trips0;
  return ORCGPU_OK;
}

// the tail: Footer, PostScript, the PostScript's length (arrow_writer.rs:130-156, :224-262)
int wr_close(orcgpu_writer* w) {
  // Footer.types, preorder: subtypes and field_names of the Structs (a List: its element; a Map: its key and value)
  PbOut types_root;
  types_root.u64(1, 12);  // STRUCT
  std::vector<uint64_t> sub;
  for (int k : w->root_kids) sub.push_back((uint64_t)k + 1);
  types_root.packed(2, sub);
  for (int k : w->root_kids) types_root.bytes(3, w->cols[(size_t)k].name.data(), w->cols[(size_t)k].name.size());
  PbOut footer;
  uint64_t body = 0, rows = 0;
  for (auto& s : w->stripes) {
    body += s.index_length + s.data_length + s.footer_length;
    rows += s.rows;
  }
  footer.u64(1, 3);
  footer.u64(2, body + 3);
  for (auto& s : w->stripes) {
    PbOut m;
    m.u64(1, s.offset);
    m.u64(2, s.index_length);
    m.u64(3, s.data_length);
    m.u64(4, s.footer_length);
    m.u64(5, s.rows);
    footer.msg(3, m);
  }
  footer.msg(4, types_root);
  for (auto& c : w->cols) {
    PbOut t;
    t.u64(1, (uint64_t)c.orc_kind);
    sub.clear();
    for (int k : c.kids) sub.push_back((uint64_t)k + 1);
    t.packed(2, sub);
    if (c.stream_kind == 7)
      for (int k : c.kids) t.bytes(3, w->cols[(size_t)k].name.data(), w->cols[(size_t)k].name.size());
    if (c.stream_kind == 6) t.u64(5, c.precision), t.u64(6, c.scale);
    footer.msg(4, t);
  }
  footer.u64(6, rows);
  const bool comp = w->comp != ORCGPU_COMP_NONE;
  PbOut metadata;
  if (w->stride) {
    // Footer.statistics: the stripes' merged; Metadata: a StripeStatistics per stripe
    std::vector<WrStat> file(w->cols.size() + 1);
    for (auto& ss : w->stripe_stats) {
      PbOut m;
      for (size_t ci = 0; ci < ss.size(); ci++) {
        m.msg(1, wr_stat_msg(ci ? &w->cols[ci - 1] : nullptr, ss[ci]));
        wr_stat_merge(file[ci], ss[ci]);
      }
      metadata.msg(1, m);
    }
    file[0].has_null = false;
    for (size_t ci = 0; ci < file.size(); ci++) footer.msg(7, wr_stat_msg(ci ? &w->cols[ci - 1] : nullptr, file[ci]));
    footer.u64(8, w->stride);
    if (comp) metadata.b = lzc_original_chunks(metadata.b, w->comp_block);
  }
  footer.u64(9, 0xffffffffull);
  if (comp) footer.b = lzc_original_chunks(footer.b, w->comp_block);
  PbOut ps;
  ps.u64(1, footer.b.size());
  ps.u64(2, (uint64_t)w->comp);  // CompressionKind (the reference: None)
  if (comp) ps.u64(3, w->comp_block);
  ps.packed(4, {0, 12});
  ps.u64(5, metadata.b.size());
  ps.u64(6, 0xffffffffull);
  ps.bytes(8000, "ORC", 3);
  int rc = wr_sink(w, metadata.b.data(), metadata.b.size());
  if (rc) return rc;
  rc = wr_sink(w, footer.b.data(), footer.b.size());
  if (rc) return rc;
  rc = wr_sink(w, ps.b.data(), ps.b.size());
  if (rc) return rc;
  const uint8_t len = (uint8_t)ps.b.size();
  return wr_sink(w, &len, 1);
}

// an upper bound of what a column's value encoder can count for n values (written out or pending)
inline uint64_t wr_bound(const WrCol& c, uint64_t n) {
  if (c.stream_kind == 5) return 2 * wr_stream_bound(0, 8, n);
  if (c.stream_kind == 6) return wr_stream_bound(0, 2, n);
  return wr_stream_bound(c.stream_kind == 1 ? 1 : 0, c.elem, n);
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

// ArrowWriter::write after orcgpu_writer_write's checks; dev_ends: the device string columns' first and last offsets.
// *rejected: the batch holds a value without an encoding (INVALID_ARGUMENT) and the writer is as it was before the call
int wr_write(orcgpu_writer* w, const struct ArrowArray* batch, uint32_t flags, const std::vector<int64_t>& dev_ends, bool* rejected) {
  orcgpu_ctx* ctx = w->ctx;
  const uint64_t R = batch->length < 0 ? 0 : (uint64_t)batch->length;
  if (batch->n_children != (int64_t)w->root_kids.size() || (w->root_kids.size() && !batch->children)) return ORCGPU_INVALID_ARGUMENT;
  if (R == 0) return ORCGPU_OK;  // (no slice: step_by over an empty range)
  if (R >= 0xffffffffull - 1024) {
    set_err(ctx, "writer: %llu rows in one batch (fewer than 2^32 - 1024 per write)", (unsigned long long)R);
    return ORCGPU_INVALID_ARGUMENT;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const bool on_device = flags & ORCGPU_ENC_ON_DEVICE;
  const uint64_t bs = w->batch_size, n_slices = (R + bs - 1) / bs;
  const size_t nc = w->cols.size();
  if (!wr_ensure(w, w->slice_counts, nc * n_slices * 16 + 16 * nc + kAlign)) return ORCGPU_HIP_ERROR;
  uint64_t* d_cv = (uint64_t*)w->slice_counts.p;  // [col][slice] valid, then [col][slice] bytes, then the columns' "bad offsets" words
  uint64_t* d_cb = d_cv + nc * n_slices;
  uint32_t* d_bad = (uint32_t*)(d_cb + nc * n_slices);  // (then the columns' "timestamp without an encoding" words)
  if (nc) WR_TRY(hipMemsetAsync(d_bad, 0, nc * 8, st));
  const int64_t row0 = batch->offset;
  std::vector<char> present0(nc);
  for (size_t ci = 0; ci < nc; ci++) present0[ci] = w->cols[ci].present;
  auto reject = [&]() {  // nothing of the batch was taken: the writer stays as it was
    for (size_t k = 0; k < nc; k++) w->cols[k].present = present0[k];
    *rejected = true;
    return ORCGPU_INVALID_ARGUMENT;
  };
  // 0. every column's array, and the rows it can hold by the host's look at its parent's two end offsets: the parent's index q
  // of a row lies in [qlo, qhi) and the row's place in the array's buffers is q + base.  The root is a Struct whose rows are
  // 0 .. R; a Struct's child has its parent's q, a List's or Map's the offsets' values [klo, khi)
  struct WrArr {
    const ArrowArray* a = nullptr;
    uint64_t base = 0;
    int64_t qlo = 0, qhi = 0, klo = 0, khi = 0;
  };
  std::vector<WrArr> A(nc);
  for (size_t ci = 0; ci < nc; ci++) {
    const WrCol& c = w->cols[ci];
    WrArr& x = A[ci];
    int64_t shift = row0;
    x.qlo = 0;
    x.qhi = (int64_t)R;
    if (c.parent < 0) {
      x.a = batch->children[c.child];
    } else {
      const WrCol& pc = w->cols[(size_t)c.parent];
      const WrArr& px = A[(size_t)c.parent];
      const ArrowArray* pa = px.a;
      if (pc.orc_kind == 11) {  // (the Map's entries: a Struct without nulls of the key and the value)
        if (pa->n_children != 1 || !pa->children || !pa->children[0] || pa->children[0]->offset < 0 || pa->children[0]->length < px.khi) return reject();
        pa = pa->children[0];
      }
      if (pa->n_children <= c.child || !pa->children) return reject();
      x.a = pa->children[c.child];
      if (pc.stream_kind == 7) shift = (int64_t)px.base, x.qlo = px.qlo, x.qhi = px.qhi;
      else shift = pc.orc_kind == 11 ? pa->offset : 0, x.qlo = px.klo, x.qhi = px.khi;
    }
    const ArrowArray* a = x.a;
    const int need = c.stream_kind == 7 ? 1 : (c.is_string ? 3 : 2);
    if (!a || a->offset < 0 || a->n_buffers < need || !a->buffers) return reject();
    if (a->length < x.qhi + shift) {
      set_err(ctx, "writer: column %zu ('%s') has %lld rows, fewer than its parent's offsets address", ci, c.path.c_str(), (long long)a->length);
      return reject();
    }
    x.base = (uint64_t)(shift + a->offset);
    const uint64_t cap = (uint64_t)(x.qhi - x.qlo);
    if (c.stream_kind != 7 && cap && (!a->buffers[1] || (c.is_string && !a->buffers[2]))) return reject();
    if (c.stream_kind == 8 && cap) {
      const uint8_t* o = (const uint8_t*)a->buffers[1];
      const uint64_t p0 = (uint64_t)x.qlo + x.base, p1 = (uint64_t)x.qhi + x.base;
      x.klo = c.elem == 4 ? (int64_t)((const int32_t*)o)[p0] : ((const int64_t*)o)[p0];
      x.khi = c.elem == 4 ? (int64_t)((const int32_t*)o)[p1] : ((const int64_t*)o)[p1];
      if (x.klo < 0 || x.khi < x.klo || (uint64_t)(x.khi - x.klo) >= 0xffffffffull - 1024) {
        set_err(ctx, "writer: the offsets of column %zu ('%s') are not ascending (or address 2^32 - 1024 rows or more)", ci, c.path.c_str());
        return reject();
      }
    }
  }
  // 1. nested schemas: the Struct / List / Map columns, parents first, without a host wait -- their presence, lengths and counts
  // per slice, and their children's rows (device/writer_nested.hip).  What comes back in one wait: NestRows per column (0: the
  // root's children), `bad`, and every column's slice ends
  struct HostRows {
    uint64_t n, start;
    bool contiguous;
  };
  std::vector<HostRows> hrows(nc + 1, HostRows{R, 0, true});
  std::vector<uint64_t> hends;  // [column + 1][slice]: rows of the column's children before each slice end
  const uint64_t* d_kends = nullptr;
  if (w->nested) {
    Bump N;
    const uint64_t o_desc = N.take((nc + 1) * sizeof(NestRows)), o_nbad = N.take(8), o_kends = N.take((nc + 1) * n_slices * 8);
    if (!wr_ensure(w, w->nest, N.off + kAlign)) return ORCGPU_HIP_ERROR;
    NestRows* d_desc = (NestRows*)(w->nest.p + o_desc);
    uint32_t* d_nbad = (uint32_t*)(w->nest.p + o_nbad);
    uint64_t* kends = (uint64_t*)(w->nest.p + o_kends);
    d_kends = kends;
    const NestRows root{R, 0, 1, 0};
    WR_TRY(hipMemsetAsync(d_nbad, 0, 8, st));
    WR_TRY(hipMemcpyAsync(d_desc, &root, sizeof root, hipMemcpyHostToDevice, st));
    WR_TRY(launch(nest_root_ends_kernel, n_slices, false, 256, st, R, bs, n_slices, kends));
    for (size_t ci = 0; ci < nc; ci++) {
      WrCol& c = w->cols[ci];
      if (!c.is_nest()) continue;
      const WrArr& x = A[ci];
      const ArrowArray* a = x.a;
      const uint8_t* validity = (const uint8_t*)a->buffers[0];
      if (validity) c.present = true;
      const bool is_list = c.stream_kind == 8;
      const uint64_t cap = (uint64_t)(x.qhi - x.qlo), lo = (uint64_t)x.qlo;
      const uint64_t kid_lo = is_list ? (uint64_t)x.klo : lo, kid_cap = is_list ? (uint64_t)(x.khi - x.klo) : cap;
      const NestRows* d_rows = d_desc + (c.parent + 1);
      const uint32_t* d_map = c.parent < 0 ? nullptr : (const uint32_t*)w->cols[(size_t)c.parent].k_map.p;
      const uint64_t* d_ends = kends + (uint64_t)(c.parent + 1) * n_slices;
      // the bytes the rows can occupy, brought over: [validity bytes][offsets]
      const uint64_t P = lo + x.base, vlo = P / 8, vhi = (P + cap + 7) / 8;
      Bump I;
      const uint64_t o_v = I.take(validity && cap ? vhi - vlo : 0), o_x = I.take(is_list && cap ? (cap + 1) * (uint64_t)c.elem : 0);
      if (!wr_ensure(w, c.b_tmp, I.off + kAlign)) return ORCGPU_HIP_ERROR;
      if (validity && cap) WR_TRY(hipMemcpyAsync(c.b_tmp.p + o_v, validity + vlo, vhi - vlo, hipMemcpyHostToDevice, st));
      if (is_list && cap)
        WR_TRY(hipMemcpyAsync(c.b_tmp.p + o_x, (const uint8_t*)a->buffers[1] + P * (uint64_t)c.elem, (cap + 1) * (uint64_t)c.elem, hipMemcpyHostToDevice, st));
      const uint8_t* d_validity = validity && cap ? c.b_tmp.p + o_v : nullptr;
      const int64_t vbit = (int64_t)x.base - (int64_t)(8 * vlo), oadj = -(int64_t)lo;
      const void* d_offsets = c.b_tmp.p + o_x;
      Bump T;
      const uint64_t n_words = (cap + 63) / 64;
      const uint64_t o_bits = T.take(n_words * 8 + 8), o_wcnt = T.take(n_words * 4), o_woff = T.take(n_words * 8), o_sums = T.take((n_words / 2048 + 2) * 8),
                     o_tot = T.take(16), o_kept = T.take(cap * 4), o_E = T.take(cap * 8 + 8), o_sums2 = T.take((cap / 2048 + 2) * 8), o_tot2 = T.take(16),
                     o_len = T.take(cap * (uint64_t)c.elem);
      if (!wr_ensure(w, c.b_bits, T.off + kAlign) || !wr_ensure(w, c.b_pres, cap + kAlign) || !wr_ensure(w, c.b_vals, cap * (uint64_t)c.elem + kAlign) ||
          !wr_ensure(w, c.k_map, kid_cap * 4 + kAlign))
        return ORCGPU_HIP_ERROR;
      uint8_t* t = c.b_bits.p;
      uint8_t* bits = t + o_bits;
      uint64_t* woff = (uint64_t*)(t + o_woff);
      uint64_t* E = (uint64_t*)(t + o_E);
      uint64_t* tot2 = (uint64_t*)(t + o_tot2);
      const int ob = is_list ? c.elem : 0;
      WR_TRY(launch(nest_kept_kernel, cap, false, 256, st, d_rows, d_map, lo, cap, d_validity, vbit, d_offsets, oadj, ob, x.klo, x.khi, c.b_pres.p,
                    (uint32_t*)(t + o_kept), (void*)(t + o_len), (const uint32_t*)d_nbad, d_nbad));
      WR_TRY(launch(enc_bytes_to_bits_kernel, (cap + 7) / 8, false, 256, st, (const uint8_t*)c.b_pres.p, cap, bits));
      WR_TRY(launch(enc_valid_counts_kernel, n_words, false, 256, st, (const uint8_t*)bits, cap, (uint32_t*)(t + o_wcnt)));
      int rc = enc_scan(ctx, st, (const uint32_t*)(t + o_wcnt), n_words, (uint64_t*)(t + o_sums), (uint64_t*)(t + o_tot), woff);
      if (rc) return rc;
      if (is_list)  // LENGTH: the valid rows' lengths
        WR_TRY(launch(enc_gather_valid_kernel, cap, false, 256, st, (const uint8_t*)bits, cap, (const uint64_t*)woff, (const void*)(t + o_len), c.elem, (void*)c.b_vals.p));
      WR_TRY(launch(nest_slice_counts_kernel, n_slices, false, 256, st, (const uint8_t*)bits, (const uint64_t*)woff, (const uint64_t*)nullptr, (const uint32_t*)nullptr, cap,
                    d_ends, n_slices, d_cv + ci * n_slices, d_cb + ci * n_slices));
      // the children's rows
      WR_TRY(hipMemsetAsync(tot2, 0, 8, st));
      rc = enc_scan(ctx, st, (const uint32_t*)(t + o_kept), cap, (uint64_t*)(t + o_sums2), tot2, E);
      if (rc) return rc;
      WR_TRY(launch(nest_desc_kernel, (uint64_t)1, true, 64, st, d_rows, d_map, lo, d_offsets, oadj, ob, (const uint64_t*)tot2, kid_cap, d_desc + (ci + 1), d_nbad));
      WR_TRY(launch(nest_fill_kernel, kid_cap, false, 256, st, d_rows, d_map, lo, d_offsets, oadj, ob, (const uint64_t*)E, (const NestRows*)(d_desc + (ci + 1)), kid_lo,
                    kid_cap, (uint32_t*)c.k_map.p, (const uint32_t*)d_nbad));
      WR_TRY(launch(nest_ends_kernel, n_slices, false, 256, st, d_ends, d_rows, (const uint64_t*)E, (const uint64_t*)tot2, n_slices, kends + (ci + 1) * n_slices,
                    (const uint32_t*)d_nbad));
    }
    std::vector<uint8_t> back(N.off);
    WR_TRY(hipMemcpyAsync(back.data(), w->nest.p, N.off, hipMemcpyDeviceToHost, st));
    int rc = wr_sync(w);
    if (rc) return rc;
    uint32_t nbad;
    memcpy(&nbad, back.data() + o_nbad, 4);
    if (nbad) {
      set_err(ctx, "writer: the offsets of a List or Map column are not ascending, or address rows beyond its child");
      return reject();
    }
    const NestRows* hd = (const NestRows*)(back.data() + o_desc);
    for (size_t k = 1; k <= nc; k++)
      if (w->cols[k - 1].is_nest()) hrows[k] = HostRows{hd[k].n, hd[k].start, hd[k].contiguous != 0};
    hends.resize((nc + 1) * n_slices);
    memcpy(hends.data(), back.data() + o_kends, (nc + 1) * n_slices * 8);
  }
  // 2. every leaf column of the batch -> presence bytes, the valid rows' values, the strings' bytes; counts per slice.  Its rows
  // are a slice of its array (below the root always; below a Struct / List when nothing was dropped), or gathered through the map
  for (size_t ci = 0; ci < nc; ci++) {
    WrCol& c = w->cols[ci];
    if (c.is_nest()) continue;
    const WrArr& x = A[ci];
    const ArrowArray* a = x.a;
    const HostRows& hr = hrows[(size_t)(c.parent + 1)];
    const uint64_t Rc = hr.n;  // the column's rows in this write
    const uint8_t* validity = (const uint8_t*)a->buffers[0];
    const uint8_t* values = (const uint8_t*)a->buffers[1];
    const uint8_t* strdata = c.is_string ? (const uint8_t*)a->buffers[2] : nullptr;
    if (validity) c.present = true;
    if (!Rc) {
      WR_TRY(hipMemsetAsync(d_cv + ci * n_slices, 0, n_slices * 8, st));
      WR_TRY(hipMemsetAsync(d_cb + ci * n_slices, 0, n_slices * 8, st));
      continue;
    }
    if (!values || (c.is_string && !strdata)) return ORCGPU_INVALID_ARGUMENT;
    if (c.parent >= 0) (hr.contiguous ? w->nested_slices : w->nested_gathers)++;
    const uint64_t off = hr.start + x.base;
    const uint64_t vb = (Rc + 7) / 8;
    // the input on the device: bits from `off`, values from `off`
    const uint8_t* d_valsrc = nullptr;  // validity bits, starting at bit d_valbit
    uint64_t d_valbit = 0;
    const uint8_t* d_values = nullptr;  // fixed width: values from row `off`; Boolean: bits (d_vbit); strings: offsets from row `off`
    uint64_t d_vbit = 0;
    const uint8_t* d_strbase = nullptr;  // strings: the byte the offsets count from
    uint64_t str_hi = 0;                 // strings: bytes addressed below offsets[off + Rc] (a bound of the valid rows' bytes)
    if (on_device) {
      d_valsrc = validity;
      d_valbit = off;
      if (c.stream_kind == 3) {
        d_values = values;
        d_vbit = off;
      } else {
        d_values = values + off * (uint64_t)c.elem;
      }
      if (c.is_string) {  // (read and checked by orcgpu_writer_write before anything changed)
        d_strbase = strdata;
        str_hi = (uint64_t)(dev_ends[2 * ci + 1] - dev_ends[2 * ci]);
      }
    } else {
      // the bytes the rows occupy, brought over: [validity bytes][values / bits / offsets][string bytes] -- the slice's, or
      // for the gather every row's the map can name: [qlo, qhi)
      const uint64_t first = hr.contiguous ? off : (uint64_t)x.qlo + x.base, count = hr.contiguous ? Rc : (uint64_t)(x.qhi - x.qlo);
      const uint64_t vlo = first / 8, vhi = (first + count + 7) / 8;
      uint64_t val_lo = 0, val_n = 0;
      int64_t s_lo = 0, s_hi = 0;
      if (c.stream_kind == 3) {
        val_lo = vlo;
        val_n = vhi - vlo;
      } else {
        val_lo = first * (uint64_t)c.elem;
        val_n = (count + (c.is_string ? 1 : 0)) * (uint64_t)c.elem;
      }
      if (c.is_string) {
        if (c.elem == 4) {
          s_lo = ((const int32_t*)values)[first];
          s_hi = ((const int32_t*)values)[first + count];
        } else {
          s_lo = ((const int64_t*)values)[first];
          s_hi = ((const int64_t*)values)[first + count];
        }
        if (s_lo < 0 || s_hi < s_lo) {
          set_err(ctx, "writer: the offsets of column %zu are not ascending", ci);
          return reject();
        }
        str_hi = (uint64_t)(s_hi - s_lo);
      }
      Bump I;
      const uint64_t o_v = I.take(validity ? vhi - vlo : 0), o_x = I.take(val_n), o_s = I.take(str_hi);
      if (!wr_ensure(w, c.b_tmp, I.off + kAlign)) return ORCGPU_HIP_ERROR;
      if (validity) WR_TRY(hipMemcpyAsync(c.b_tmp.p + o_v, validity + vlo, vhi - vlo, hipMemcpyHostToDevice, st));
      if (val_n) WR_TRY(hipMemcpyAsync(c.b_tmp.p + o_x, values + val_lo, val_n, hipMemcpyHostToDevice, st));
      if (str_hi) WR_TRY(hipMemcpyAsync(c.b_tmp.p + o_s, strdata + s_lo, str_hi, hipMemcpyHostToDevice, st));
      if (hr.contiguous) {
        d_valsrc = validity ? c.b_tmp.p + o_v : nullptr;
        d_valbit = off & 7;
        d_values = c.b_tmp.p + o_x;
        d_vbit = off & 7;
        d_strbase = c.b_tmp.p + o_s - s_lo;  // (addressed at offsets >= s_lo only)
      } else {
        // the gather: the column's ORC rows as an array of their own -- validity, values (Boolean: bits), offsets + bytes
        const uint32_t* d_map = (const uint32_t*)w->cols[(size_t)c.parent].k_map.p;  // q - qlo: the copies' row
        const int64_t bit_adj = (int64_t)(first - 8 * vlo);
        Bump Gt;
        const uint64_t o_gv = Gt.take(vb + 16), o_gx = Gt.take(c.stream_kind == 3 ? vb + 16 : (Rc + 1) * (uint64_t)c.elem + 16), o_gs = Gt.take(str_hi),
                       o_gl = Gt.take(c.is_string ? Rc * 4 : 0), o_gd = Gt.take(c.is_string ? Rc * 8 : 0), o_gsum = Gt.take((Rc / 2048 + 2) * 8), o_gtot = Gt.take(16);
        if (!wr_ensure(w, c.b_gath, Gt.off + kAlign)) return ORCGPU_HIP_ERROR;
        uint8_t* g = c.b_gath.p;
        if (validity) WR_TRY(launch(nest_gather_bits_kernel, vb, false, 256, st, d_map, Rc, (const uint8_t*)(c.b_tmp.p + o_v), bit_adj, g + o_gv));
        const uint8_t* src = c.b_tmp.p + o_x;
        const uint64_t n16 = (Rc * (uint64_t)c.elem + 15) / 16;
        if (c.stream_kind == 3) {
          WR_TRY(launch(nest_gather_bits_kernel, vb, false, 256, st, d_map, Rc, src, bit_adj, g + o_gx));
        } else if (c.is_string) {
          WR_TRY(launch(nest_str_lengths_kernel, Rc, false, 256, st, d_map, Rc, (const void*)src, c.elem, (int64_t)s_lo, (int64_t)s_hi, (uint32_t*)(g + o_gl), d_bad + ci));
          int rc = enc_scan(ctx, st, (const uint32_t*)(g + o_gl), Rc, (uint64_t*)(g + o_gsum), (uint64_t*)(g + o_gtot), (uint64_t*)(g + o_gd));
          if (rc) return rc;
          WR_TRY(launch(nest_str_copy_kernel, (Rc + 3) / 4, true, 256, st, d_map, Rc, (const void*)src, c.elem, (const uint64_t*)(g + o_gd), (const uint32_t*)(g + o_gl),
                        (const uint8_t*)(c.b_tmp.p + o_s - s_lo), g + o_gs, str_hi, (void*)(g + o_gx)));
        } else if (c.elem == 1) {
          WR_TRY(launch(nest_gather_kernel<uint8_t>, n16, false, 256, st, d_map, Rc, (const uint8_t*)src, (Nest16*)(g + o_gx)));
        } else if (c.elem == 2) {
          WR_TRY(launch(nest_gather_kernel<uint16_t>, n16, false, 256, st, d_map, Rc, (const uint16_t*)src, (Nest16*)(g + o_gx)));
        } else if (c.elem == 4) {
          WR_TRY(launch(nest_gather_kernel<uint32_t>, n16, false, 256, st, d_map, Rc, (const uint32_t*)src, (Nest16*)(g + o_gx)));
        } else if (c.elem == 8) {
          WR_TRY(launch(nest_gather_kernel<uint64_t>, n16, false, 256, st, d_map, Rc, (const uint64_t*)src, (Nest16*)(g + o_gx)));
        } else {
          WR_TRY(launch(nest_gather_kernel<Nest16>, n16, false, 256, st, d_map, Rc, (const Nest16*)src, (Nest16*)(g + o_gx)));
        }
        d_valsrc = validity ? g + o_gv : nullptr;
        d_values = g + o_gx;
        d_strbase = g + o_gs;
      }
    }
    // presence: a bitmap from bit 0 (all set without a validity buffer) and its bytes
    Bump T;
    const uint64_t n_words = (Rc + 63) / 64;
    if (c.stream_kind == 6) str_hi = Rc * (uint64_t)WR_DEC_MAX_BYTES;  // (the varints' bytes: a bound)
    const uint64_t o_bits = T.take(n_words * 8 + 8), o_vbits = T.take(c.stream_kind == 3 ? n_words * 8 + 8 : 0), o_wcnt = T.take(n_words * 4),
                   o_woff = T.take(n_words * 8), o_sums = T.take((n_words / 2048 + 2) * 8), o_tot = T.take(16),
                   o_len = T.take(c.is_string ? Rc * (uint64_t)c.elem : 0), o_vlen = T.take(c.has_bytes() ? Rc * 4 : 0),
                   o_dst = T.take(c.has_bytes() ? Rc * 8 : 0), o_sums2 = T.take((Rc / 2048 + 2) * 8), o_tot2 = T.take(16);
    if (!wr_ensure(w, c.b_bits, T.off + kAlign) || !wr_ensure(w, c.b_pres, Rc + kAlign) || !wr_ensure(w, c.b_vals, (c.stream_kind == 6 && !w->stride ? 0 : Rc * (uint64_t)c.elem) + kAlign) ||
        !wr_ensure(w, c.b_data, str_hi + kAlign) || !wr_ensure(w, c.b_vals2, (c.stream_kind == 5 ? Rc * 8 : 0) + kAlign))
      return ORCGPU_HIP_ERROR;
    uint8_t* t = c.b_bits.p;
    uint8_t* bits = t + o_bits;
    uint64_t* woff = (uint64_t*)(t + o_woff);
    WR_TRY(launch(wr_bits_kernel, vb, false, 256, st, d_valsrc, d_valbit, Rc, bits));
    WR_TRY(launch(wr_bits_to_bytes_kernel, Rc, false, 256, st, (const uint8_t*)bits, Rc, c.b_pres.p));
    WR_TRY(launch(enc_valid_counts_kernel, n_words, false, 256, st, (const uint8_t*)bits, Rc, (uint32_t*)(t + o_wcnt)));
    int rc = enc_scan(ctx, st, (const uint32_t*)(t + o_wcnt), n_words, (uint64_t*)(t + o_sums), (uint64_t*)(t + o_tot), woff);
    if (rc) return rc;
    const uint64_t* row_dst = nullptr;
    const uint32_t* vlen = nullptr;
    if (c.stream_kind == 3) {  // the valid rows' Boolean values as 0 / 1 bytes
      WR_TRY(launch(wr_bits_kernel, vb, false, 256, st, (const uint8_t*)d_values, d_vbit, Rc, t + o_vbits));
      WR_TRY(launch(enc_gather_valid_kernel, Rc, false, 256, st, (const uint8_t*)bits, Rc, (const uint64_t*)woff, (const void*)(t + o_vbits), 0, (void*)c.b_vals.p));
    } else if (c.stream_kind == 5) {  // the valid rows' seconds since 2015 and nanosecond codes
      WR_TRY(launch(wr_timestamp_kernel, Rc, false, 256, st, (const uint8_t*)bits, Rc, (const uint64_t*)woff, (const int64_t*)d_values, c.ups, c.npu,
                    (int64_t*)c.b_vals.p, (uint64_t*)c.b_vals2.p, d_bad + nc + ci));
    } else if (c.stream_kind == 6) {  // the valid rows' varints one behind the other, and the values themselves (statistics)
      WR_TRY(launch(wr_dec_lengths_kernel, Rc, false, 256, st, (const uint64_t*)d_values, (const uint8_t*)bits, Rc, (uint32_t*)(t + o_vlen)));
      rc = enc_scan(ctx, st, (const uint32_t*)(t + o_vlen), Rc, (uint64_t*)(t + o_sums2), (uint64_t*)(t + o_tot2), (uint64_t*)(t + o_dst));
      if (rc) return rc;
      WR_TRY(launch(wr_dec_pack_kernel, (Rc + 255) / 256, true, 256, st, (const uint64_t*)d_values, (const uint8_t*)bits, Rc, (const uint64_t*)(t + o_dst),
                    (const uint32_t*)(t + o_vlen), c.b_data.p, str_hi));
      if (w->stride)  // (the values themselves: only the row index statistics read them)
        WR_TRY(launch(enc_gather_valid_kernel, Rc, false, 256, st, (const uint8_t*)bits, Rc, (const uint64_t*)woff, (const void*)d_values, 16, (void*)c.b_vals.p));
      row_dst = (const uint64_t*)(t + o_dst);
      vlen = (const uint32_t*)(t + o_vlen);
    } else if (!c.is_string) {
      WR_TRY(launch(enc_gather_valid_kernel, Rc, false, 256, st, (const uint8_t*)bits, Rc, (const uint64_t*)woff, (const void*)d_values, c.elem, (void*)c.b_vals.p));
    } else {
      WR_TRY(launch(enc_lengths_kernel, Rc, false, 256, st, (const void*)d_values, c.elem, (const uint8_t*)bits, Rc, (void*)(t + o_len), (uint32_t*)(t + o_vlen),
                    d_bad + ci));
      rc = enc_scan(ctx, st, (const uint32_t*)(t + o_vlen), Rc, (uint64_t*)(t + o_sums2), (uint64_t*)(t + o_tot2), (uint64_t*)(t + o_dst));
      if (rc) return rc;
      // (bounded by str_hi: the offsets are checked when the counts come back, `bad`)
      WR_TRY(launch(wr_copy_strings_kernel, (Rc + 3) / 4, true, 256, st, (const uint8_t*)bits, (const void*)d_values, c.elem, Rc, (const uint64_t*)(t + o_dst),
                    d_strbase, c.b_data.p, str_hi));
      WR_TRY(launch(enc_gather_valid_kernel, Rc, false, 256, st, (const uint8_t*)bits, Rc, (const uint64_t*)woff, (const void*)(t + o_len), c.elem, (void*)c.b_vals.p));
      row_dst = (const uint64_t*)(t + o_dst);
      vlen = (const uint32_t*)(t + o_vlen);
    }
    if (w->nested)
      WR_TRY(launch(nest_slice_counts_kernel, n_slices, false, 256, st, (const uint8_t*)bits, (const uint64_t*)woff, row_dst, vlen, Rc,
                    d_kends + (uint64_t)(c.parent + 1) * n_slices, n_slices, d_cv + ci * n_slices, d_cb + ci * n_slices));
    else
      WR_TRY(launch(wr_slice_counts_kernel, n_slices, false, 256, st, (const uint8_t*)bits, (const uint64_t*)woff, row_dst, vlen, Rc, bs, n_slices, d_cv + ci * n_slices,
                    d_cb + ci * n_slices));
  }
  std::vector<uint64_t> cv(nc * n_slices), cb(nc * n_slices);
  std::vector<uint32_t> bad(2 * nc);
  if (nc) {
    WR_TRY(hipMemcpyAsync(cv.data(), d_cv, nc * n_slices * 8, hipMemcpyDeviceToHost, st));
    WR_TRY(hipMemcpyAsync(cb.data(), d_cb, nc * n_slices * 8, hipMemcpyDeviceToHost, st));
    WR_TRY(hipMemcpyAsync(bad.data(), d_bad, nc * 8, hipMemcpyDeviceToHost, st));
  }
  int rc = wr_sync(w);
  if (rc) return rc;
  for (size_t ci = 0; ci < nc; ci++)
    if (bad[ci]) {
      set_err(ctx, "writer: the offsets of column %zu are not ascending (or a value is 4 GiB or longer)", ci);
      return w->nested ? reject() : ORCGPU_INVALID_ARGUMENT;
    }
  for (size_t ci = 0; ci < nc; ci++)
    if (bad[nc + ci]) {  // nothing of the batch was taken: the writer stays as it was
      set_err(ctx, "writer: column %zu holds a timestamp ORC cannot encode (within the second before 1970-01-01 00:00:00 but not on it, or its second too far from 2015 for i64)", ci);
      return reject();
    }
  auto V = [&](size_t ci, uint64_t j) -> uint64_t { return j ? cv[ci * n_slices + j - 1] : 0; };  // valid rows before slice j
  auto B = [&](size_t ci, uint64_t j) -> uint64_t { return j ? cb[ci * n_slices + j - 1] : 0; };
  auto rows_to = [&](uint64_t j) -> uint64_t { return std::min<uint64_t>(j * bs, R); };        // rows before slice j
  // ... and a column's own rows before it: its parent's children's
  auto RT = [&](size_t ci, uint64_t j) -> uint64_t {
    if (!w->nested) return rows_to(j);
    return j ? hends[(size_t)(w->cols[ci].parent + 1) * n_slices + j - 1] : 0;
  };
  // the stripe's buffers extended by the batch's slices [j0, j1) (the counters move only with `commit`)
  auto extend = [&](uint64_t j0, uint64_t j1, bool commit) -> int {
    for (size_t ci = 0; ci < nc; ci++) {
      WrCol& c = w->cols[ci];
      const uint64_t dv = V(ci, j1) - V(ci, j0), dr = RT(ci, j1) - RT(ci, j0), db = B(ci, j1) - B(ci, j0);
      const uint64_t velem = c.stream_kind == 6 && !w->stride ? 0 : (uint64_t)c.elem;  // (Decimal128 values: kept for the row index only)
      const uint64_t nv = c.n_valid * velem, add = dv * velem;
      if (velem && !wr_reserve(w, c.vals, nv + add + kAlign, nv)) return ORCGPU_HIP_ERROR;
      if (add) WR_TRY(hipMemcpyAsync(c.vals.p + nv, c.b_vals.p + V(ci, j0) * velem, add, hipMemcpyDeviceToDevice, st));
      if (c.stream_kind == 5 || c.stream_kind == 6) {
        const uint64_t e2 = (uint64_t)c.elem2(), nv2 = c.n_valid * e2;
        if (!wr_reserve(w, c.vals2, nv2 + dv * e2 + kAlign, nv2)) return ORCGPU_HIP_ERROR;
        if (dv && c.stream_kind == 5) WR_TRY(hipMemcpyAsync(c.vals2.p + nv2, c.b_vals2.p + V(ci, j0) * e2, dv * e2, hipMemcpyDeviceToDevice, st));
        if (dv && c.stream_kind == 6) WR_TRY(launch(wr_fill16_kernel, dv, false, 256, st, (uint16_t*)(c.vals2.p + nv2), dv, (uint16_t)c.scale));
      }
      if (commit) {
        if (!wr_reserve(w, c.pres, c.rows + dr + kAlign, c.rows)) return ORCGPU_HIP_ERROR;
        if (dr) WR_TRY(hipMemcpyAsync(c.pres.p + c.rows, c.b_pres.p + RT(ci, j0), dr, hipMemcpyDeviceToDevice, st));
        if (c.has_bytes()) {
          if (!wr_reserve(w, c.data, c.n_bytes + db + kAlign, c.n_bytes)) return ORCGPU_HIP_ERROR;
          if (db) WR_TRY(hipMemcpyAsync(c.data.p + c.n_bytes, c.b_data.p + B(ci, j0), db, hipMemcpyDeviceToDevice, st));
        }
        c.rows += dr;
        c.n_valid += dv;
        c.n_bytes += db;
      }
    }
    if (commit) w->rows += rows_to(j1) - rows_to(j0);
    return ORCGPU_OK;
  };
  // the summed estimate after slice j (j0 <= j) of the terms that are counts: floats, Booleans, string bytes, PRESENT
  auto counted = [&](uint64_t j0, uint64_t j, uint64_t* rle_bound) -> uint64_t {
    uint64_t e = 0, bound = 0;
    for (size_t ci = 0; ci < nc; ci++) {
      const WrCol& c = w->cols[ci];
      const uint64_t nv = c.n_valid + V(ci, j + 1) - V(ci, j0);
      if (c.present) e += (c.rows + RT(ci, j + 1) - RT(ci, j0)) / 8;
      switch (c.stream_kind) {
        case 2: e += nv * (uint64_t)c.elem; break;
        case 3: e += nv / 8; break;
        case 7: break;
        // (the run-length encoded terms: exactly base_rle when the columns had base_valid values; each run written out since
        // covers values from then on, or from the run open then -- at most 512 values before)
        case 4: case 6: e += c.n_bytes + B(ci, j + 1) - B(ci, j0); bound += wr_bound(c, nv - c.base_valid + 512); break;
        default: bound += wr_bound(c, nv - c.base_valid + 512); break;
      }
    }
    if (rle_bound) *rle_bound = w->base_rle + bound;
    return e;
  };
  // the first slice in [j0, j1) after which the estimate exceeds the limit, or j1
  std::vector<uint64_t> est;  // the run-length encoded terms after the analysed slices
  auto analyse = [&](uint64_t j0, uint64_t j1) -> int64_t {
    const uint64_t win = j1 - j0;
    if (!wr_ensure(w, w->est, win * 8 + kAlign)) return -1;
    uint64_t* d_est = (uint64_t*)w->est.p;
    if (hipMemsetAsync(d_est, 0, win * 8, st) != hipSuccess) return -1;
    if (extend(j0, j1, false)) return -1;
    for (size_t ci = 0; ci < nc; ci++) {
      WrCol& c = w->cols[ci];
      if (c.stream_kind == 2 || c.stream_kind == 3 || c.stream_kind == 7) continue;
      // which of the column's value streams go through an encoder: Timestamp both (as two Int64 columns would count),
      // Decimal128 the second alone (the scale; its DATA bytes are counted), every other column its one
      const int first = c.stream_kind == 6, last = c.stream_kind == 5 || c.stream_kind == 6;
      for (int second = first; second <= last; second++) {
        EncJob J;
        J.kind = c.stream_kind == 1 ? 1 : 0;
        J.int_bytes = second ? c.elem2() : c.elem;
        J.is_signed = second ? c.stream_kind == 6 : (c.stream_kind == 0 || c.stream_kind == 5);
        J.n = c.n_valid + V(ci, j1) - V(ci, j0);
        J.values = second ? c.vals2.p : c.vals.p;
        J.deferred = true;  // (no host wait: the run count stays on the device, the grids cover n runs)
        J.syncs = &w->round_trips;
        if (!J.n) continue;
        if (!wr_ensure(w, w->trig, J.n * 8 + kAlign)) return -1;  // (before the plan: growing waits, and the tables are the plan's)
        if (enc_plan(ctx, J)) return -1;
        uint64_t* d_trig = (uint64_t*)w->trig.p;
        hipError_t e = J.kind == 0 ? launch(wr_triggers_kernel<0>, (uint64_t)J.n_runs, false, 256, st, (const void*)J.values, J.int_bytes, (const uint32_t*)J.runs,
                                            J.d_n_runs, J.n, d_trig)
                                   : launch(wr_triggers_kernel<1>, (uint64_t)J.n_runs, false, 256, st, (const void*)J.values, 1, (const uint32_t*)J.runs, J.d_n_runs,
                                            J.n, d_trig);
        if (e != hipSuccess) return -1;
        // values after slice j: c.n_valid + cv[j] - V(j0)
        e = launch(wr_estimate_kernel, win, false, 256, st, (const uint64_t*)d_trig, (const uint32_t*)J.runs, (const uint32_t*)J.run_bytes, (const uint64_t*)J.offsets,
                   J.d_n_runs, J.kind, (const uint64_t*)(d_cv + ci * n_slices + j0), (int64_t)c.n_valid - (int64_t)V(ci, j0), win, d_est);
        if (e != hipSuccess) return -1;
      }
    }
    est.assign(win, 0);
    if (hipMemcpyAsync(est.data(), d_est, win * 8, hipMemcpyDeviceToHost, st) != hipSuccess || wr_sync(w)) return -1;
    for (uint64_t j = j0; j < j1; j++)
      if (est[j - j0] + counted(j0, j, nullptr) > w->stripe_byte_size) return (int64_t)j;
    return (int64_t)j1;
  };
  uint64_t j0 = 0;
  while (j0 < n_slices) {
    // slices that cannot reach the limit by the bound: taken as they are
    uint64_t js = j0;
    while (js < n_slices) {
      uint64_t bound;
      const uint64_t e = counted(j0, js, &bound);
      if (e + bound > w->stripe_byte_size) break;
      js++;
    }
    if (js == n_slices) {
      rc = extend(j0, n_slices, true);
      if (rc) return rc;
      break;
    }
    // the rest: windows of the run analysis, growing
    uint64_t win = std::max<uint64_t>(w->window_hint, js - j0 + 1);
    int64_t cut;
    for (;;) {
      const uint64_t j1 = std::min<uint64_t>(n_slices, j0 + win);
      cut = analyse(j0, j1);
      if (cut < 0) {
        if (ctx->err.empty()) set_err(ctx, "writer: the stripe analysis failed");
        return ORCGPU_HIP_ERROR;
      }
      if ((uint64_t)cut < j1 || j1 == n_slices) break;
      win *= 2;
    }
    if ((uint64_t)cut == n_slices) {
      rc = extend(j0, n_slices, true);
      if (rc) return rc;
      w->base_rle = est.back();  // (exact at the end of this write: later bounds start from it)
      for (auto& c : w->cols) c.base_valid = c.n_valid;
      break;
    }
    rc = extend(j0, (uint64_t)cut + 1, true);
    if (rc) return rc;
    rc = wr_flush(w);
    if (rc) return rc;
    w->window_hint = std::max<uint64_t>(1, (uint64_t)cut + 1 - j0);
    j0 = (uint64_t)cut + 1;
  }
  return wr_sync(w);  // (the caller may release the batch now)
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
    int rc = wr_read_schema(ctx, schema, fields, md, fl);
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
        if (a && a->offset >= 0 && batch->offset >= 0 && a->length >= batch->offset + R && a->n_buffers >= (c.stream_kind == 7 ? 1 : 2) && a->buffers) continue;
        set_err(ctx, "writer: column %zu of the batch is not an Arrow array of its type", ci);
        return ORCGPU_INVALID_ARGUMENT;
      }
      if (!a || a->offset < 0 || batch->offset < 0 || a->length < batch->offset + R || a->n_buffers < (c.is_string ? 3 : 2) || !a->buffers ||
          !a->buffers[1] || (c.is_string && !a->buffers[2])) {
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
  w->stride = stride;
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
  for (auto& c : w->cols) {
    c.pres.release();
    c.vals.release();
    c.vals2.release();
    c.data.release();
    c.b_bits.release();
    c.b_pres.release();
    c.b_vals.release();
    c.b_vals2.release();
    c.b_data.release();
    c.b_tmp.release();
    c.k_map.release();
    c.b_gath.release();
    c.b_dict.release();
  }
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
