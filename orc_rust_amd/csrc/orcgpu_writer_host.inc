// orcgpu_writer_host.inc -- the ArrowWriter's host code that never touches the device (orcgpu_writer.inc holds what does): free
// of HIP, it compiles with a plain C++17 compiler, and tests/hostcheck/writer_host_check.cpp compiles this very text under
// AddressSanitizer + UBSan.
//
//   PbOut                       a protobuf message being written
//   WrCol, wr_column_of,        a column's plain description, and the only place that maps an Arrow format to (kind, element
//   wr_add_column               width, ORC type, encoding); the schema -> the column tree, preorder
//   wr_streams                  ONE description of a column's streams: which, from which buffer, through which encoder, with
//                               which row index positions, counted how toward the stripe estimate
//   WrStat, wr_stat_merge,      ColumnStatistics: the device's records (device/writer_kinds.h: IxRec) merged and written
//   wr_stat_msg, wr_*_bound
//   wr_row_index,               the bytes of a stripe's ROW_INDEX streams, its footer and the file's tail
//   wr_stripe_footer, wr_tail
//   wr_bloom_size,              Bloom filters (orcgpu_writer_set_bloom_filter): Apache ORC's sizing, and a column's
//   wr_bloom_stream             BLOOM_FILTER_UTF8 stream around the bitsets the device built (device/bloom_build.hip)
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/orcgpu.h"
#include "arrow_c_data.h"
#include "device/writer_kinds.h"

namespace {

void wr_errf(std::string& err, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  err = buf;
}

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

// ORC framing of bytes stored as they are: original chunks of at most B bytes (the writer's index streams, stripe footers and tail)
std::vector<uint8_t> wr_original_chunks(const std::vector<uint8_t>& b, uint64_t B) {
  std::vector<uint8_t> out;
  out.reserve(b.size() + 3 * ((b.size() + B - 1) / B));
  for (uint64_t at = 0; at < b.size(); at += B) {
    const uint64_t len = std::min<uint64_t>(B, b.size() - at);
    const uint64_t h = len * 2 + 1;
    out.push_back((uint8_t)h);
    out.push_back((uint8_t)(h >> 8));
    out.push_back((uint8_t)(h >> 16));
    out.insert(out.end(), b.begin() + at, b.begin() + at + len);
  }
  return out;
}

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

// a column's plain description (its device buffers: WrColDev, orcgpu_writer.inc)
struct WrCol {
  int elem = 0;        // bytes of a value as the column's value encoder takes it (Boolean: a byte; strings and Lists: the offset width)
  bool is_string = false;
  int stream_kind = WR_INT;  // WrKind
  int orc_kind = 0;    // Type.Kind (ORCGPU_T_*)
  int encoding = 0;    // ColumnEncoding.Kind (ORCGPU_ENC_*) of a stripe that writes no dictionary for it
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
  // dictionary (orcgpu_writer_set_dictionary): the stripe being flushed -- whether the column is written DICTIONARY_V2, its
  // entries and their bytes
  bool dict = false;
  uint64_t dict_size = 0, dict_bytes = 0;
  bool bloom = false;  // a BLOOM_FILTER_UTF8 stream behind the column's ROW_INDEX (orcgpu_writer_set_bloom_filter)
  bool is_nest() const { return stream_kind == WR_STRUCT || stream_kind == WR_LIST; }
  bool has_bytes() const { return stream_kind == WR_STRING || stream_kind == WR_DECIMAL; }  // n_bytes / data count toward the estimate
  bool is_utf8() const { return orc_kind == ORCGPU_T_STRING; }  // a string column with a minimum / maximum, and the one a dictionary is tried for
  int elem2() const { return stream_kind == WR_TIMESTAMP ? 8 : 2; }  // bytes of a value of the second value stream (vals2)
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

// the column writer of an Arrow leaf type (writer/stripe.rs:173-187, arrow_writer.rs:158-222); false: the reference's unimplemented!()
bool wr_column_of(const char* fmt, WrCol& c) {
  auto set = [&c](int elem, int kind, int orc, int enc) {
    c.elem = elem; c.stream_kind = kind; c.orc_kind = orc; c.encoding = enc; c.is_string = kind == WR_STRING;
    return true;
  };
  if (!fmt || !fmt[0]) return false;
  if (fmt[0] == 't' && fmt[1] == 's' && fmt[2] && fmt[3] == ':') {  // Timestamp(unit, tz): with a zone an instant
    switch (fmt[2]) {
      case 's': c.ups = 1; c.npu = 1000000000; break;
      case 'm': c.ups = 1000; c.npu = 1000000; break;
      case 'u': c.ups = 1000000; c.npu = 1000; break;
      case 'n': c.ups = 1000000000; c.npu = 1; break;
      default: return false;
    }
    return set(8, WR_TIMESTAMP, fmt[4] ? ORCGPU_T_TIMESTAMP_INSTANT : ORCGPU_T_TIMESTAMP, ORCGPU_ENC_DIRECT_V2);
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
    c.precision = (uint32_t)p; c.scale = (uint32_t)sc;
    return set(16, WR_DECIMAL, ORCGPU_T_DECIMAL, ORCGPU_ENC_DIRECT_V2);
  }
  if (fmt[1]) return false;
  switch (fmt[0]) {
    case 'b': return set(1, WR_BOOL, ORCGPU_T_BOOLEAN, ORCGPU_ENC_DIRECT);
    case 'c': return set(1, WR_BYTE, ORCGPU_T_BYTE, ORCGPU_ENC_DIRECT);
    case 's': return set(2, WR_INT, ORCGPU_T_SHORT, ORCGPU_ENC_DIRECT_V2);
    case 'i': return set(4, WR_INT, ORCGPU_T_INT, ORCGPU_ENC_DIRECT_V2);
    case 'l': return set(8, WR_INT, ORCGPU_T_LONG, ORCGPU_ENC_DIRECT_V2);
    case 'f': return set(4, WR_FLOAT, ORCGPU_T_FLOAT, ORCGPU_ENC_DIRECT);
    case 'g': return set(8, WR_FLOAT, ORCGPU_T_DOUBLE, ORCGPU_ENC_DIRECT);
    case 'u': return set(4, WR_STRING, ORCGPU_T_STRING, ORCGPU_ENC_DIRECT_V2);
    case 'U': return set(8, WR_STRING, ORCGPU_T_STRING, ORCGPU_ENC_DIRECT_V2);
    case 'z': return set(4, WR_STRING, ORCGPU_T_BINARY, ORCGPU_ENC_DIRECT_V2);
    case 'Z': return set(8, WR_STRING, ORCGPU_T_BINARY, ORCGPU_ENC_DIRECT_V2);
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

int wr_read_schema(std::string& err, const ArrowSchema* s, std::vector<WrField>& fields, std::string& md, int64_t& flags) {
  if (!s || !s->format || strcmp(s->format, "+s") != 0 || s->n_children < 0 || (s->n_children && !s->children)) {
    wr_errf(err, "writer: the schema must be an Arrow struct (format \"+s\") of its fields");
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

// the columns of a schema: every column of the tree but the root, preorder
struct WrTree {
  std::vector<WrCol> cols;
  std::vector<int> root_kids;
  bool nested = false;  // a Struct, List or Map column among them
};

int wr_unsupported(std::string& err, const WrField& f, const std::string& path, const char* why) {
  wr_errf(err, "writer: unsupported Arrow type '%s' of field '%s'%s (the reference: unimplemented!(\"unsupported datatype\"), writer/stripe.rs:186; beyond it: Timestamp, Decimal128, Struct, List, LargeList, Map)",
          f.format.c_str(), path.c_str(), why);
  return ORCGPU_UNSUPPORTED;
}

// a field and what is below it -> columns, preorder.  +s STRUCT, +l / +L LIST, +m MAP (its key and value: the entries struct
// gets no column); under_list: below a List or Map, where Decimal128 is not written
int wr_add_column(std::string& err, WrTree& t, const WrField& f, int parent, int child, const std::string& path, bool under_list) {
  const char* fmt = f.format.c_str();
  if (f.dictionary) return wr_unsupported(err, f, path, " (dictionary encoded)");
  WrCol c;
  const std::vector<WrField>* kids = nullptr;
  if (!strcmp(fmt, "+s")) {
    c.elem = 0; c.stream_kind = WR_STRUCT; c.orc_kind = ORCGPU_T_STRUCT; c.encoding = ORCGPU_ENC_DIRECT;
    kids = &f.kids;
  } else if (!strcmp(fmt, "+l") || !strcmp(fmt, "+L")) {
    if (f.kids.size() != 1) return ORCGPU_INVALID_ARGUMENT;
    c.elem = fmt[1] == 'l' ? 4 : 8; c.stream_kind = WR_LIST; c.orc_kind = ORCGPU_T_LIST; c.encoding = ORCGPU_ENC_DIRECT_V2;
    kids = &f.kids;
    under_list = true;
  } else if (!strcmp(fmt, "+m")) {
    if (f.kids.size() != 1 || f.kids[0].format != "+s" || f.kids[0].kids.size() != 2) return ORCGPU_INVALID_ARGUMENT;
    c.elem = 4; c.stream_kind = WR_LIST; c.orc_kind = ORCGPU_T_MAP; c.encoding = ORCGPU_ENC_DIRECT_V2;
    kids = &f.kids[0].kids;
    under_list = true;
  } else if (fmt[0] == '+') {  // FixedSizeList, ListView, Union, run-end encoded
    return wr_unsupported(err, f, path, "");
  } else {
    if (!wr_column_of(fmt, c)) return wr_unsupported(err, f, path, "");
    if (c.stream_kind == WR_DECIMAL && under_list) return wr_unsupported(err, f, path, " (Decimal128 below a List or Map)");
  }
  c.name = f.name;
  c.path = path;
  c.parent = parent;
  c.child = child;
  const int me = (int)t.cols.size();
  t.cols.push_back(std::move(c));
  if (parent >= 0) t.cols[(size_t)parent].kids.push_back(me);
  else t.root_kids.push_back(me);
  if (kids) {
    t.nested = true;
    for (size_t i = 0; i < kids->size(); i++) {
      const int rc = wr_add_column(err, t, (*kids)[i], me, (int)i, path + "." + (*kids)[i].name, under_list);
      if (rc) return rc;
    }
  }
  return ORCGPU_OK;
}

int wr_tree_of(std::string& err, const std::vector<WrField>& fields, WrTree& t) {
  for (size_t i = 0; i < fields.size(); i++) {
    const int rc = wr_add_column(err, t, fields[i], -1, (int)i, fields[i].name, false);
    if (rc) {
      if (rc == ORCGPU_INVALID_ARGUMENT) wr_errf(err, "writer: field '%s' is not a well-formed Arrow type", fields[i].name.c_str());
      return rc;
    }
  }
  return ORCGPU_OK;
}

// ---- a column's streams ------------------------------------------------------------------------------------------------------
// the ONE description of which streams a column writes: the flush enqueues them from it, the stripe cut prices them from it.
// In the stripe's stream order per column (writer/stripe.rs:128-150): the value streams, then PRESENT.
enum WrSrc { WR_SRC_VALS, WR_SRC_VALS2, WR_SRC_DATA, WR_SRC_PRES, WR_SRC_DICT_IDS, WR_SRC_DICT_LEN, WR_SRC_DICT_DATA };  // WrColDev's buffers
enum WrEnc { WR_ENC_RLE2, WR_ENC_BYTE_RLE, WR_ENC_BITS, WR_ENC_COPY };  // Integer RLE v2; byte RLE; bits over byte RLE; the bytes as they are
enum WrCost { WR_COST_COUNT, WR_COST_RUNS };  // toward the stripe estimate: a count of bytes, or what the encoder's runs come to
constexpr int WR_NO_POS = -1;
constexpr int WR_MAX_STREAMS = 4;

struct WrStream {
  int stream;     // Stream.Kind (ORCGPU_S_*)
  int src;        // WrSrc
  uint64_t n;     // items: values (RLE2, BYTE_RLE), bits (BITS), bytes (COPY)
  int enc;        // WrEnc
  int width;      // RLE2 / BYTE_RLE: bytes of a value
  int is_signed;  // RLE2
  int pos_mode;   // row index: ix_pos_kernel's mode, or WR_NO_POS (nothing in the row index)
  int pos_form;   // ... 1 bytes, 2 run-length, 3 bits over byte runs
  int cost;       // WrCost
};

// the stripe's counts a description is made for: the open stripe's, or what they would be after more slices
struct WrCounts {
  uint64_t rows, n_valid, n_bytes;
};

int wr_streams(const WrCol& c, const WrCounts& k, bool indexed, WrStream out[WR_MAX_STREAMS]) {
  int n = 0;
  auto rle2 = [&](int stream, int src, uint64_t items, int width, int is_signed, bool positions = true) {
    out[n++] = WrStream{stream, src, items, WR_ENC_RLE2, width, is_signed, positions ? 1 : WR_NO_POS, 2, WR_COST_RUNS};
  };
  auto copy = [&](int stream, int src, uint64_t bytes, int pos_mode) {
    out[n++] = WrStream{stream, src, bytes, WR_ENC_COPY, 0, 0, pos_mode, 1, WR_COST_COUNT};
  };
  switch (c.stream_kind) {
    case WR_INT: rle2(ORCGPU_S_DATA, WR_SRC_VALS, k.n_valid, c.elem, 1); break;
    case WR_BYTE: out[n++] = WrStream{ORCGPU_S_DATA, WR_SRC_VALS, k.n_valid, WR_ENC_BYTE_RLE, 1, 0, 2, 2, WR_COST_RUNS}; break;
    case WR_FLOAT: copy(ORCGPU_S_DATA, WR_SRC_VALS, k.n_valid * (uint64_t)c.elem, 4); break;
    case WR_BOOL: out[n++] = WrStream{ORCGPU_S_DATA, WR_SRC_VALS, k.n_valid, WR_ENC_BITS, 1, 0, 3, 3, WR_COST_COUNT}; break;
    case WR_STRING:
      if (c.dict) {
        // DICTIONARY_V2: DATA the rows' ids (positions as an integer column's), LENGTH the entries' lengths, DICTIONARY_DATA their
        // bytes; the row index holds nothing for the last two
        rle2(ORCGPU_S_DATA, WR_SRC_DICT_IDS, k.n_valid, c.elem, 0);
        rle2(ORCGPU_S_LENGTH, WR_SRC_DICT_LEN, c.dict_size, c.elem, 0, false);
        copy(ORCGPU_S_DICTIONARY_DATA, WR_SRC_DICT_DATA, c.dict_bytes, WR_NO_POS);
      } else {
        copy(ORCGPU_S_DATA, WR_SRC_DATA, k.n_bytes, 5);
        rle2(ORCGPU_S_LENGTH, WR_SRC_VALS, k.n_valid, c.elem, 0);
      }
      break;
    case WR_TIMESTAMP:  // the seconds (signed); SECONDARY: the nanosecond codes (unsigned)
      rle2(ORCGPU_S_DATA, WR_SRC_VALS, k.n_valid, 8, 1);
      rle2(ORCGPU_S_SECONDARY, WR_SRC_VALS2, k.n_valid, c.elem2(), 0);
      break;
    case WR_DECIMAL:  // the varints; SECONDARY: the scale (signed)
      copy(ORCGPU_S_DATA, WR_SRC_DATA, k.n_bytes, 5);
      rle2(ORCGPU_S_SECONDARY, WR_SRC_VALS2, k.n_valid, c.elem2(), 1);
      break;
    case WR_STRUCT: break;  // PRESENT alone
    case WR_LIST: rle2(ORCGPU_S_LENGTH, WR_SRC_VALS, k.n_valid, c.elem, 0, false); break;
  }
  if (c.present) out[n++] = WrStream{ORCGPU_S_PRESENT, WR_SRC_PRES, k.rows, WR_ENC_BITS, 1, 0, 0, 3, WR_COST_COUNT};
  if (!indexed)
    for (int i = 0; i < n; i++) out[i].pos_mode = WR_NO_POS;
  return n;
}
inline WrCounts wr_counts(const WrCol& c) { return WrCounts{c.rows, c.n_valid, c.n_bytes}; }
// the buffer the row index statistics read beside the values: the nanosecond codes, else the strings' bytes
inline int wr_stats_src(const WrCol& c) { return c.stream_kind == WR_TIMESTAMP ? WR_SRC_VALS2 : WR_SRC_DATA; }

// an upper bound of an encoded stream of n values (RLE v2: a run of one value is 2 header bytes + the value, a DELTA of three
// values a header, two varints of up to 10 bytes and the packed delta, PATCHED_BASE adds its patch list; byte RLE: a header byte
// per value and the value)
inline uint64_t wr_stream_bound(int enc, int width, uint64_t n) { return enc == WR_ENC_BYTE_RLE ? 2 * n + 2 : (uint64_t)(3 * width + 12) * n + 64; }
inline uint64_t wr_bits_bytes(uint64_t bits) { return (bits + 7) / 8; }

// what a stream adds to the stripe estimate as a count (WR_COST_COUNT), and an upper bound of what its encoder can count for n
// values, written out or pending (WR_COST_RUNS)
inline uint64_t wr_counted(const WrStream& s) { return s.cost != WR_COST_COUNT ? 0 : (s.enc == WR_ENC_BITS ? s.n / 8 : s.n); }
inline uint64_t wr_runs_bound(const WrStream& s, uint64_t n) { return s.cost != WR_COST_RUNS ? 0 : wr_stream_bound(s.enc, s.width, n); }

// ---- row index: statistics on the host ------------------------------------------------------------------------------------
// a group's record as the device wrote it; side: the string copies
WrStat wr_stat_of(const WrCol& c, const IxRec& r, const uint8_t* side) {
  WrStat s;
  s.count = r.count;
  s.has_null = r.has_null != 0;
  if (!r.count) return s;
  switch (c.stream_kind) {
    case WR_INT: case WR_BYTE:
      s.imin = r.imin;
      s.imax = r.imax;
      s.isum = (__int128)(((unsigned __int128)(uint64_t)r.sum_hi << 64) | r.sum_lo);
      break;
    case WR_FLOAT: s.dmin = r.dmin; s.dmax = r.dmax; s.dsum = r.dsum; s.dsum_lo = r.dsum_lo; s.dbig = r.dbig; s.dbig_lo = r.dbig_lo; s.has_nan = r.has_nan != 0; break;
    case WR_BOOL: s.trues = r.trues; break;
    case WR_TIMESTAMP: s.imin = r.imin; s.imax = r.imax; s.nmin = (uint32_t)r.sum_lo; s.nmax = (uint32_t)r.sum_hi; break;
    case WR_DECIMAL:
      s.qmin = (__int128)(((unsigned __int128)(uint64_t)r.imax << 64) | (uint64_t)r.imin);
      s.qmax = (__int128)(((unsigned __int128)r.smax_at << 64) | r.smin_at);
      s.qsum[0] = r.sum_lo, s.qsum[1] = (uint64_t)r.sum_hi, s.qsum[2] = r.trues, s.qsum[3] = (uint64_t)((int64_t)r.trues >> 63);
      break;
    default:
      s.bytes = r.bytes;
      if (c.is_utf8()) {
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
#ifdef __clang__
#pragma clang fp contract(off)
#endif
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
  size_t cut = std::min<size_t>(1024, s.size());
  while (cut > 0 && cut < s.size() && ((uint8_t)s[cut] & 0xc0) == 0x80) cut--;
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
#ifdef __clang__
#pragma clang fp contract(off)
#endif
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
      case WR_INT: case WR_BYTE:
        t.sint(1, s.imin);
        t.sint(2, s.imax);
        if (s.isum >= (__int128)INT64_MIN && s.isum <= (__int128)INT64_MAX) t.sint(3, (int64_t)s.isum);
        m.msg(2, t);
        break;
      case WR_FLOAT:
        if (s.has_nan) break;  // (no DoubleStatistics: a reader would take an absent bound for 0)
        t.f64(1, s.dmin);
        t.f64(2, s.dmax);
        t.f64(3, wr_float_sum(s));
        m.msg(3, t);
        break;
      case WR_BOOL:
        t.packed(1, {s.trues});
        m.msg(5, t);
        break;
      case WR_TIMESTAMP: {  // TimestampStatistics: floor milliseconds (the writer's zone is UTC: the legacy fields hold the same), and the
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
      case WR_DECIMAL: {  // DecimalStatistics: the sum when |sum| < 10^38
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
        if (c->orc_kind == ORCGPU_T_BINARY) {
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

// ---- the bytes the host writes ----------------------------------------------------------------------------------------------
struct WrStreamOut {  // a stream of the stripe being flushed: its slot in the device buffer the encoders write to
  int kind;           // Stream.Kind
  uint32_t column;
  uint64_t slot;
};

// a stripe's ROW_INDEX streams, column 0 (the root) first, and its statistics [column], from what the device brought back: the
// (column, group) records, the streams' positions and the string copies.  ix_streams[column]: its streams (index, position form)
// in the order the positions list them: PRESENT, then the value streams
std::vector<std::vector<uint8_t>> wr_row_index(const std::vector<WrCol>& cols, uint64_t rows, uint64_t S, uint64_t G, const IxRec* recs, const uint64_t* pos,
                                               const uint8_t* side, const std::vector<std::vector<std::pair<uint64_t, int>>>& ix_streams, bool comp,
                                               uint64_t comp_block, std::vector<WrStat>& stripe) {
  const size_t nc = cols.size();
  std::vector<std::vector<uint8_t>> index;
  stripe.assign(nc + 1, WrStat());
  stripe[0].count = rows;
  PbOut root;
  for (uint64_t g = 0; g < G; g++) {
    WrStat s;
    s.count = std::min(S, rows - g * S);
    PbOut e;
    e.msg(2, wr_stat_msg(nullptr, s));
    root.msg(1, e);
  }
  index.push_back(root.b);
  for (size_t ci = 0; ci < nc; ci++) {
    PbOut ri;
    std::vector<uint64_t> p;
    for (uint64_t g = 0; g < G; g++) {
      const WrStat s = wr_stat_of(cols[ci], recs[ci * G + g], side);
      wr_stat_merge(stripe[ci + 1], s);
      p.clear();
      wr_positions(pos, G, g, comp, ix_streams[ci], p);
      PbOut e;
      e.packed(1, p);
      e.msg(2, wr_stat_msg(&cols[ci], s));
      ri.msg(1, e);
    }
    index.push_back(ri.b);
  }
  if (comp)
    for (auto& b : index) b = wr_original_chunks(b, comp_block);
  return index;
}

// ---- Bloom filters ------------------------------------------------------------------------------------------------------------
// Apache ORC's sizing (BloomFilter.java: optimalNumOfBits, optimalNumOfHashFunctions) for n = the row index stride expected
// entries and the false positive probability fpp in (0, 1): the bitset's 64-bit words, and k hash functions
void wr_bloom_size(uint64_t n, double fpp, uint64_t& words, uint32_t& k) {
  const double bits = std::floor(-(double)n * std::log(fpp) / (std::log(2.0) * std::log(2.0)));  // (int64) of a value >= 0
  words = (uint64_t)(bits / 64.0) + 1;
  const double kk = std::floor(bits / (double)n * std::log(2.0) + 0.5);  // Math.round
  k = kk < 1.0 ? 1u : (kk > 4294967295.0 ? 4294967295u : (uint32_t)kk);
}

// a column's BLOOM_FILTER_UTF8 stream: a BloomFilterIndex of G BloomFilter {1 numHashFunctions, 3 utf8bitset}; bitsets: G times
// `words` u64 as the device left them (word w: 8 little-endian bytes at utf8bitset[8w]).  Its length depends on (words, k, G) alone
std::vector<uint8_t> wr_bloom_stream(uint32_t k, uint64_t words, uint64_t G, const uint8_t* bitsets, bool comp, uint64_t comp_block) {
  PbOut head;  // what precedes a filter's bitset bytes
  head.u64(1, k);
  head.key(3, 2);
  head.varint(words * 8);
  PbOut out;
  out.b.reserve(G * (words * 8 + head.b.size() + 8));
  for (uint64_t g = 0; g < G; g++) {
    out.key(1, 2);
    out.varint(head.b.size() + words * 8);
    out.b.insert(out.b.end(), head.b.begin(), head.b.end());
    out.b.insert(out.b.end(), bitsets + g * words * 8, bitsets + (g + 1) * words * 8);
  }
  return comp ? wr_original_chunks(out.b, comp_block) : out.b;
}

// StripeFooter: the index streams -- per column its ROW_INDEX, then its BLOOM_FILTER_UTF8 (bloom[column], of the columns that
// have one: WrCol::bloom) --, the data streams with their lengths, the columns' encodings (column 0 the root)
std::vector<uint8_t> wr_stripe_footer(const std::vector<WrCol>& cols, const std::vector<std::vector<uint8_t>>& index, const std::vector<WrStreamOut>& streams,
                                      const std::vector<uint64_t>& lens, bool comp, uint64_t comp_block,
                                      const std::vector<std::vector<uint8_t>>& bloom = std::vector<std::vector<uint8_t>>()) {
  PbOut footer;
  for (size_t ci = 0; ci < index.size(); ci++) {
    PbOut m;
    m.u64(1, ORCGPU_S_ROW_INDEX);
    m.u64(2, ci);
    m.u64(3, index[ci].size());
    footer.msg(1, m);
    if (ci && cols[ci - 1].bloom && ci < bloom.size()) {
      PbOut b;
      b.u64(1, ORCGPU_S_BLOOM_FILTER_UTF8);
      b.u64(2, ci);
      b.u64(3, bloom[ci].size());
      footer.msg(1, b);
    }
  }
  for (size_t i = 0; i < streams.size(); i++) {
    PbOut m;
    m.u64(1, (uint64_t)streams[i].kind);
    m.u64(2, streams[i].column);
    m.u64(3, lens[i]);
    footer.msg(1, m);
  }
  for (size_t ci = 0; ci <= cols.size(); ci++) {
    PbOut m;
    m.u64(1, ci ? (uint64_t)(cols[ci - 1].dict ? ORCGPU_ENC_DICTIONARY_V2 : cols[ci - 1].encoding) : (uint64_t)ORCGPU_ENC_DIRECT);
    if (ci && cols[ci - 1].dict) m.u64(2, cols[ci - 1].dict_size);
    footer.msg(2, m);
  }
  for (auto& c : cols)
    if (c.stream_kind == WR_TIMESTAMP) {  // (without it Apache ORC reads TIMESTAMP columns in the reading host's zone)
      footer.bytes(3, "UTC", 3);
      break;
    }
  return comp ? wr_original_chunks(footer.b, comp_block) : footer.b;
}

// the tail: Metadata, Footer, PostScript, the PostScript's length (arrow_writer.rs:130-156, :224-262).  stripe_stats: [stripe][column],
// column 0 the root, of a writer with a row index (stride > 0)
std::vector<uint8_t> wr_tail(const std::vector<WrCol>& cols, const std::vector<int>& root_kids, const std::vector<WrStripe>& stripes,
                             const std::vector<std::vector<WrStat>>& stripe_stats, uint64_t stride, int comp_kind, uint64_t comp_block) {
  // Footer.types, preorder: subtypes and field_names of the Structs (a List: its element; a Map: its key and value)
  PbOut types_root;
  types_root.u64(1, ORCGPU_T_STRUCT);
  std::vector<uint64_t> sub;
  for (int k : root_kids) sub.push_back((uint64_t)k + 1);
  types_root.packed(2, sub);
  for (int k : root_kids) types_root.bytes(3, cols[(size_t)k].name.data(), cols[(size_t)k].name.size());
  PbOut footer;
  uint64_t body = 0, rows = 0;
  for (auto& s : stripes) {
    body += s.index_length + s.data_length + s.footer_length;
    rows += s.rows;
  }
  footer.u64(1, 3);
  footer.u64(2, body + 3);
  for (auto& s : stripes) {
    PbOut m;
    m.u64(1, s.offset);
    m.u64(2, s.index_length);
    m.u64(3, s.data_length);
    m.u64(4, s.footer_length);
    m.u64(5, s.rows);
    footer.msg(3, m);
  }
  footer.msg(4, types_root);
  for (auto& c : cols) {
    PbOut t;
    t.u64(1, (uint64_t)c.orc_kind);
    sub.clear();
    for (int k : c.kids) sub.push_back((uint64_t)k + 1);
    t.packed(2, sub);
    if (c.stream_kind == WR_STRUCT)
      for (int k : c.kids) t.bytes(3, cols[(size_t)k].name.data(), cols[(size_t)k].name.size());
    if (c.stream_kind == WR_DECIMAL) t.u64(5, c.precision), t.u64(6, c.scale);
    footer.msg(4, t);
  }
  footer.u64(6, rows);
  const bool comp = comp_kind != ORCGPU_COMP_NONE;
  PbOut metadata;
  if (stride) {
    // Footer.statistics: the stripes' merged; Metadata: a StripeStatistics per stripe
    std::vector<WrStat> file(cols.size() + 1);
    for (auto& ss : stripe_stats) {
      PbOut m;
      for (size_t ci = 0; ci < ss.size(); ci++) {
        m.msg(1, wr_stat_msg(ci ? &cols[ci - 1] : nullptr, ss[ci]));
        wr_stat_merge(file[ci], ss[ci]);
      }
      metadata.msg(1, m);
    }
    file[0].has_null = false;
    for (size_t ci = 0; ci < file.size(); ci++) footer.msg(7, wr_stat_msg(ci ? &cols[ci - 1] : nullptr, file[ci]));
    footer.u64(8, stride);
    if (comp) metadata.b = wr_original_chunks(metadata.b, comp_block);
  }
  footer.u64(9, 0xffffffffull);
  if (comp) footer.b = wr_original_chunks(footer.b, comp_block);
  PbOut ps;
  ps.u64(1, footer.b.size());
  ps.u64(2, (uint64_t)comp_kind);  // CompressionKind (the reference: None)
  if (comp) ps.u64(3, comp_block);
  ps.packed(4, {0, 12});
  ps.u64(5, metadata.b.size());
  ps.u64(6, 0xffffffffull);
  ps.bytes(8000, "ORC", 3);
  std::vector<uint8_t> out = std::move(metadata.b);
  out.insert(out.end(), footer.b.begin(), footer.b.end());
  out.insert(out.end(), ps.b.begin(), ps.b.end());
  out.push_back((uint8_t)ps.b.size());
  return out;
}

}  // namespace
