// orcgpu_meta.inc -- the host-side parsers of the ORC container, PURE C++ (no HIP, no device, no context): the protobuf wire
// reader, PostScript / Footer / StripeFooter / RowIndex parsing, the type-tree validation, row-index entry splitting, the column
// shard's weights and deal, and (orcgpu_predicate.inc) row-group statistics, Bloom filters and predicate evaluation.
//
//   read_metadata                    src/reader/metadata.rs:180-247 (PostScript, Footer; hand-written protobuf wire reader:
//                                    format/orc_proto.proto, SURVEY Appendix C)
//   Stripe::new / StreamMap          src/stripe.rs:127-182, :311-336
//   RowIndex                         src/row_index.rs:204-330
//
// Included by orcgpu_reader_meta.inc and orcgpu_reader_plan.inc (the product: liborcgpu.so) AND by tests/hostcheck/hostcheck.cpp, which compiles exactly this
// text with g++ -fsanitize=address,undefined and feeds it the fixture files and their mutations on the CPU
// (tests/test_host_sanitized.py) -- everything here parses UNTRUSTED bytes.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include <sys/mman.h>
#include <unistd.h>

namespace orcgpu_host {

// ---- protobuf wire reader ------------------------------------------------------------------------------
struct PbField {
  uint32_t num;
  uint32_t wt;
  uint64_t v;           // varint / fixed value
  const uint8_t* p;     // length-delimited payload
  uint64_t n;
};
struct PbReader {
  const uint8_t* p;
  const uint8_t* end;
  bool ok = true;
  PbReader(const uint8_t* b, uint64_t n) : p(b), end(b + n) {}
  bool varint(uint64_t* out) {
    uint64_t v = 0;
    int s = 0;
    while (p < end) {
      uint8_t c = *p++;
      v |= (uint64_t)(c & 0x7f) << s;
      s += 7;
      if (!(c & 0x80)) {
        *out = v;
        return true;
      }
      if (s > 63) break;
    }
    ok = false;
    return false;
  }
  bool next(PbField& f) {
    if (p >= end || !ok) return false;
    uint64_t key;
    if (!varint(&key)) return false;
    f.num = (uint32_t)(key >> 3);
    f.wt = (uint32_t)(key & 7);
    f.v = 0;
    f.p = nullptr;
    f.n = 0;
    if (f.wt == 0) return varint(&f.v);
    if (f.wt == 2) {
      uint64_t n;
      if (!varint(&n) || n > (uint64_t)(end - p)) {
        ok = false;
        return false;
      }
      f.p = p;
      f.n = n;
      p += n;
      return true;
    }
    uint64_t w = f.wt == 1 ? 8 : (f.wt == 5 ? 4 : 0);
    if (!w || w > (uint64_t)(end - p)) {
      ok = false;
      return false;
    }
    memcpy(&f.v, p, w);
    p += w;
    return true;
  }
};

}  // namespace orcgpu_host
#include "orcgpu_predicate.inc"
namespace orcgpu_host {

// what went wrong, for the caller to pass on (the product: orcgpu_last_error)
struct MetaErr {
  char msg[512] = {0};  // (as long as the context keeps: orcgpu_last_error)
  void set(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
  }
};

// ---- ChunkReader (reader/mod.rs:27-76) ------------------------------------------------------------------
struct ChunkReader {
  virtual ~ChunkReader() {}
  virtual uint64_t len() const = 0;
  virtual bool get_bytes(uint64_t off, uint64_t n, std::vector<uint8_t>& out) = 0;
  // the bytes where they lie, if the source has them in memory (else null: get_bytes): stream bytes then go to the staging
  // pipeline without a copy of their own
  virtual const uint8_t* view(uint64_t off, uint64_t n) const { (void)off; (void)n; return nullptr; }
};
struct FileChunkReader : ChunkReader {
  FILE* f = nullptr;
  uint64_t size = 0;
  const uint8_t* map = nullptr;  // the file mapped read-only (null: it could not be): what stream bytes are staged from
  explicit FileChunkReader(const char* path) {
    f = fopen(path, "rb");
    if (f) {
      fseek(f, 0, SEEK_END);
      size = (uint64_t)ftell(f);
      if (size && !getenv("ORCGPU_NO_MMAP")) {  // (a file that may shrink while it is read: ORCGPU_NO_MMAP=1 reads it with fread)
        void* m = mmap(nullptr, (size_t)size, PROT_READ, MAP_PRIVATE, fileno(f), 0);
        if (m != MAP_FAILED) {
          map = static_cast<const uint8_t*>(m);
          (void)madvise(m, (size_t)size, MADV_SEQUENTIAL);
        }
      }
    }
  }
  ~FileChunkReader() override {
    if (map) (void)munmap(const_cast<uint8_t*>(map), (size_t)size);
    if (f) fclose(f);
  }
  uint64_t len() const override { return size; }
  const uint8_t* view(uint64_t off, uint64_t n) const override { return map && off <= size && n <= size - off ? map + off : nullptr; }
  bool get_bytes(uint64_t off, uint64_t n, std::vector<uint8_t>& out) override {
    if (!f || off > size || n > size - off) return false;  // (no wrap: both come from the untrusted footer)
    out.resize(n);
    if (fseeko(f, (off_t)off, SEEK_SET)) return false;
    return n == 0 || fread(out.data(), 1, n, f) == n;
  }
};
struct BytesChunkReader : ChunkReader {
  std::vector<uint8_t> data;
  BytesChunkReader(const uint8_t* p, uint64_t n) : data(p, p + n) {}
  uint64_t len() const override { return data.size(); }
  const uint8_t* view(uint64_t off, uint64_t n) const override { return off <= data.size() && n <= data.size() - off ? data.data() + off : nullptr; }
  bool get_bytes(uint64_t off, uint64_t n, std::vector<uint8_t>& out) override {
    if (off > data.size() || n > data.size() - off) return false;  // (no wrap: both come from the untrusted footer)
    out.assign(data.begin() + off, data.begin() + off + n);
    return true;
  }
};

// ---- file metadata (reader/metadata.rs, schema.rs) --------------------------------------------------------
struct OrcType {
  int kind = 12;
  std::vector<uint32_t> subtypes;
  std::vector<std::string> field_names;
  uint32_t precision = 0, scale = 0;
};
struct StripeInfo {
  uint64_t offset = 0, index_length = 0, data_length = 0, footer_length = 0, number_of_rows = 0;
};
struct FileMetadata {
  int compression = 0;
  uint64_t block_size = 262144;
  uint64_t number_of_rows = 0;
  uint64_t row_index_stride = 10000;  // Footer.rowIndexStride; the default per the ORC specification (stripe.rs:300)
  std::vector<OrcType> types;
  std::vector<StripeInfo> stripes;
};
struct StreamInfo {
  int kind;
  uint32_t column;
  uint64_t length;
  uint64_t offset;  // absolute file offset
};
// RowIndex of one column of one stripe (row_index.rs:204-226): the positions of every RowIndexEntry, back to back
struct ColumnIndex {
  uint32_t column = 0;
  uint32_t n_groups = 0, per_group = 0;  // per_group = 0: the entries differ in length (not usable)
  std::vector<uint64_t> positions;
  bool has_groups = false;               // statistics and Bloom filters of the row groups (read for a predicate)
  ColumnGroups groups;
};
struct StripeFooter {
  std::vector<ColumnIndex> index;   // of the projected columns, when the reader prunes row groups (read_stripe_index)
  bool index_read = false;
  std::vector<StreamInfo> streams;
  std::vector<std::pair<int, uint32_t>> encodings;  // (kind, dictionary_size) by column id
  std::string writer_timezone;
  bool has_tz = false;
};

// Well-formed UTF-8 (what prost demands of a protobuf `string`): no stray continuation bytes, no overlong forms, no surrogates,
// nothing above U+10FFFF.
bool utf8_ok(const uint8_t* p, size_t n) {
  size_t i = 0;
  while (i < n) {
    const uint8_t c = p[i];
    if (c < 0x80) {
      i++;
      continue;
    }
    size_t len;
    uint32_t cp, lo;
    if ((c & 0xe0) == 0xc0) len = 2, cp = c & 0x1f, lo = 0x80;
    else if ((c & 0xf0) == 0xe0) len = 3, cp = c & 0x0f, lo = 0x800;
    else if ((c & 0xf8) == 0xf0) len = 4, cp = c & 0x07, lo = 0x10000;
    else return false;
    if (i + len > n) return false;
    for (size_t k = 1; k < len; k++) {
      if ((p[i + k] & 0xc0) != 0x80) return false;
      cp = (cp << 6) | (p[i + k] & 0x3f);
    }
    if (cp < lo || cp > 0x10ffff || (cp >= 0xd800 && cp <= 0xdfff)) return false;
    i += len;
  }
  return true;
}

// PostScript (the file's last bytes in front of its length byte; metadata.rs:192-215).  `tail` = the file's last bytes (up to
// DEFAULT_FOOTER_SIZE of them).
int parse_postscript(const uint8_t* tail_p, uint64_t tail_n, FileMetadata& md, uint64_t& ps_len, uint64_t& footer_length, MetaErr& err) {
  if (!tail_n) return ORCGPU_OUT_OF_SPEC;
  struct Tail {
    const uint8_t* p;
    uint64_t n;
    uint8_t back() const { return p[n - 1]; }
    uint64_t size() const { return n; }
    const uint8_t* data() const { return p; }
  } tail{tail_p, tail_n};
  ps_len = tail.back();
  if (tail.size() - 1 < ps_len) {
    err.set("File too small for given postscript length");
    return ORCGPU_OUT_OF_SPEC;
  }
  uint64_t metadata_length = 0;
  footer_length = 0;
  bool has_fl = false, has_ml = false, has_bs = false;
  {
    PbReader pr(tail.data() + tail.size() - 1 - ps_len, ps_len);
    PbField f;
    while (pr.next(f)) {
      if (f.num == 1 && f.wt == 0) footer_length = f.v, has_fl = true;
      else if (f.num == 2 && f.wt == 0) md.compression = (int)f.v;
      else if (f.num == 3 && f.wt == 0) md.block_size = f.v, has_bs = true;
      else if (f.num == 5 && f.wt == 0) metadata_length = f.v, has_ml = true;
    }
    // (footerLength and metadataLength are optional fields: the reference reads a missing one as 0 -- files of Hive 0.11 carry no
    // metadata length, tests/integration/data/orc_no_format.orc --; a footer of no bytes then fails for want of types)
    (void)has_ml;
    if (!pr.ok || !has_fl) {
      err.set("malformed PostScript");
      return ORCGPU_OUT_OF_SPEC;
    }
    if (!has_bs) md.block_size = 262144;  // compression.rs:31
  }
  (void)metadata_length;
  return ORCGPU_OK;
}

// Footer (metadata.rs:217-247; format/orc_proto.proto Footer): stripes, types, row count, row index stride.
int parse_footer(const uint8_t* footer_p, uint64_t footer_n, FileMetadata& md, MetaErr& err) {
  struct Bytes {
    const uint8_t* p;
    uint64_t n;
    const uint8_t* data() const { return p; }
    uint64_t size() const { return n; }
  } footer{footer_p, footer_n};
  PbReader pr(footer.data(), footer.size());
  PbField f;
  while (pr.next(f)) {
    if (f.num == 3 && f.wt == 2) {
      StripeInfo si;
      PbReader q(f.p, f.n);
      PbField g;
      while (q.next(g)) {
        if (g.num == 1) si.offset = g.v;
        else if (g.num == 2) si.index_length = g.v;
        else if (g.num == 3) si.data_length = g.v;
        else if (g.num == 4) si.footer_length = g.v;
        else if (g.num == 5) si.number_of_rows = g.v;
      }
      md.stripes.push_back(si);
    } else if (f.num == 4 && f.wt == 2) {
      OrcType t;
      t.kind = 0;
      PbReader q(f.p, f.n);
      PbField g;
      while (q.next(g)) {
        if (g.num == 1) t.kind = (int)g.v;
        else if (g.num == 2) {
          if (g.wt == 0) t.subtypes.push_back((uint32_t)g.v);
          else {
            PbReader pk(g.p, g.n);
            uint64_t v;
            while (pk.p < pk.end && pk.varint(&v)) t.subtypes.push_back((uint32_t)v);
          }
        } else if (g.num == 3 && g.wt == 2) {
          // (a protobuf `string`: the reference's decoder rejects a name that is not UTF-8)
          if (!utf8_ok(g.p, (size_t)g.n)) {
            err.set("malformed Footer: a field name is not UTF-8");
            return ORCGPU_OUT_OF_SPEC;
          }
          t.field_names.emplace_back((const char*)g.p, (size_t)g.n);
        }
        else if (g.num == 5) t.precision = (uint32_t)g.v;
        else if (g.num == 6) t.scale = (uint32_t)g.v;
      }
      // (`#[prost(enumeration = "r#type::Kind", optional, tag = "1")]`, proto.rs:349: the accessor the reference reads a type's kind through
      // gives the enumeration's default -- Boolean, its first variant -- for a number that names no variant; so does this reader: a type
      // of kind 67 is a Boolean column to both.  Left as it was, the kind fell through every switch of the planner: a List / Map whose
      // child had such a kind was exported without the child, which no consumer of the C Data Interface imports)
      if (t.kind < 0 || t.kind > ORCGPU_T_TIMESTAMP_INSTANT) t.kind = ORCGPU_T_BOOLEAN;
      md.types.push_back(std::move(t));
    } else if (f.num == 6 && f.wt == 0) {
      md.number_of_rows = f.v;
    } else if (f.num == 8 && f.wt == 0) {
      md.row_index_stride = f.v;
    }
  }
  if (!pr.ok) {
    err.set("malformed Footer");
    return ORCGPU_OUT_OF_SPEC;
  }
  // The type list is a tree in preorder (what the reference's schema builder assumes, schema.rs): every subtype id lies behind its
  // parent's and inside the list, and no type has two parents.  Checked once, here: the walks over the tree (reader_build,
  // type_weight) then visit every type at most once -- a crafted list like k -> [k + 1, k + 1] would cost them 2^depth visits.
  {
    std::vector<uint8_t> seen(md.types.size(), 0);
    for (size_t id = 0; id < md.types.size(); id++)
      for (uint32_t k : md.types[id].subtypes) {
        if (k <= id || k >= md.types.size() || seen[k]) {
          err.set("malformed Footer: type %zu names subtype %u (%s)", id, k, k <= id ? "not behind its parent" : (k >= md.types.size() ? "outside the type list" : "a second parent"));
          return ORCGPU_OUT_OF_SPEC;
        }
        seen[k] = 1;
      }
  }
  return ORCGPU_OK;
}

// The bytes of a stripe's footer as the file holds them.
int stripe_footer_raw(ChunkReader& r, const StripeInfo& si, std::vector<uint8_t>& raw, MetaErr& err) {
  // StripeInformation comes from the untrusted file footer: no sum may wrap, every part lies inside the file
  const uint64_t flen = r.len();
  if (si.offset > flen || si.index_length > flen - si.offset || si.data_length > flen - si.offset - si.index_length ||
      si.footer_length > flen - si.offset - si.index_length - si.data_length) {
    err.set("stripe at %llu reaches beyond the end of the file", (unsigned long long)si.offset);
    return ORCGPU_OUT_OF_SPEC;
  }
  return r.get_bytes(si.offset + si.index_length + si.data_length, si.footer_length, raw) ? ORCGPU_OK : ORCGPU_IO_ERROR;
}

// StripeFooter (proto) -> the stripe's streams with their places in the file, its columns' encodings, its time zone
// StripeFooter (proto) -> the stripe's streams with their places in the file, its columns' encodings, its time zone
int parse_stripe_footer(const StripeInfo& si, const std::vector<uint8_t>& plain, StripeFooter& sf, MetaErr& err) {
  const uint64_t stripe_end = si.offset + si.index_length + si.data_length;
  PbReader pr(plain.data(), plain.size());
  PbField f;
  uint64_t off = si.offset;  // streams are laid out from the stripe start, index streams first (stripe.rs:154-165)
  while (pr.next(f)) {
    if (f.num == 1 && f.wt == 2) {
      StreamInfo s{0, 0, 0, 0};
      PbReader q(f.p, f.n);
      PbField g;
      while (q.next(g)) {
        if (g.num == 1) s.kind = (int)g.v;
        else if (g.num == 2) s.column = (uint32_t)g.v;
        else if (g.num == 3) s.length = g.v;
      }
      if (s.length > stripe_end - off) {  // (the running offset never leaves the stripe, so it cannot wrap either)
        err.set("a stream of the stripe at %llu reaches beyond the stripe's data", (unsigned long long)si.offset);
        return ORCGPU_OUT_OF_SPEC;
      }
      s.offset = off;
      off += s.length;
      sf.streams.push_back(s);
    } else if (f.num == 2 && f.wt == 2) {
      int kind = 0;
      uint32_t dsz = 0;
      PbReader q(f.p, f.n);
      PbField g;
      while (q.next(g)) {
        if (g.num == 1) kind = (int)g.v;
        else if (g.num == 2) dsz = (uint32_t)g.v;
      }
      sf.encodings.emplace_back(kind, dsz);
    } else if (f.num == 3 && f.wt == 2) {
      sf.writer_timezone.assign((const char*)f.p, (size_t)f.n);
      sf.has_tz = true;
    }
  }
  return pr.ok ? ORCGPU_OK : ORCGPU_OUT_OF_SPEC;
}


struct IndexSections {  // one stripe's index streams among the raw sections of a decompress call
  size_t base = 0, n_index = 0, n = 0;  // raws[base .. base+n): n_index ROW_INDEX streams, then the Bloom filter streams
  std::vector<uint32_t> cols;           // per ROW_INDEX stream: its column
  std::vector<int> bloom_of;            // per ROW_INDEX stream: its Bloom filter stream, counted from base (-1: none)
};
int index_gather(ChunkReader& r, const StripeFooter& sf, const std::vector<uint32_t>& columns, bool want_stats,
                 std::vector<std::vector<uint8_t>>& raws, IndexSections& is) {
  is.base = raws.size();
  for (auto& s : sf.streams) {
    if (s.kind != ORCGPU_S_ROW_INDEX || std::find(columns.begin(), columns.end(), s.column) == columns.end()) continue;
    raws.emplace_back();
    if (!r.get_bytes(s.offset, s.length, raws.back())) return ORCGPU_IO_ERROR;
    is.cols.push_back(s.column);
  }
  is.n_index = raws.size() - is.base;
  is.bloom_of.assign(is.n_index, -1);
  if (want_stats)
    for (size_t k = 0; k < is.n_index; k++)
      for (int kind : {ORCGPU_S_BLOOM_FILTER, ORCGPU_S_BLOOM_FILTER_UTF8}) {
        if (is.bloom_of[k] >= 0) break;
        for (auto& s : sf.streams)
          if (s.kind == kind && s.column == is.cols[k]) {
            is.bloom_of[k] = (int)(raws.size() - is.base);
            raws.emplace_back();
            if (!r.get_bytes(s.offset, s.length, raws.back())) return ORCGPU_IO_ERROR;
            break;
          }
      }
  is.n = raws.size() - is.base;
  return ORCGPU_OK;
}
int index_parse(StripeFooter& sf, const IndexSections& is, const std::vector<std::vector<uint8_t>>& plains, bool want_stats) {
  for (size_t k = 0; k < is.n_index; k++) {
    const std::vector<uint8_t>& plain = plains[is.base + k];
    ColumnIndex ci;
    ci.column = is.cols[k];
    bool uniform = true, first = true;
    PbReader pr(plain.data(), plain.size());
    PbField f;
    while (pr.next(f)) {
      if (f.num != 1 || f.wt != 2) continue;  // RowIndex.entry
      PbReader q(f.p, f.n);
      PbField g;
      uint32_t n_pos = 0;
      while (q.next(g)) {
        if (g.num != 1) continue;  // RowIndexEntry.positions (packed, or one varint per field)
        if (g.wt == 0) {
          ci.positions.push_back(g.v);
          n_pos++;
        } else if (g.wt == 2) {
          PbReader pk(g.p, g.n);
          uint64_t v;
          while (pk.p < pk.end && pk.varint(&v)) {
            ci.positions.push_back(v);
            n_pos++;
          }
        }
      }
      if (!q.ok) return ORCGPU_OUT_OF_SPEC;
      if (first) ci.per_group = n_pos;
      else if (n_pos != ci.per_group) uniform = false;
      first = false;
      ci.n_groups++;
    }
    if (!pr.ok) return ORCGPU_OUT_OF_SPEC;
    if (!uniform) ci.per_group = 0;
    if (want_stats) {
      const std::vector<uint8_t>* bl = is.bloom_of[k] >= 0 ? &plains[is.base + is.bloom_of[k]] : nullptr;
      ci.has_groups = parse_column_groups(plain.data(), plain.size(), bl ? bl->data() : nullptr, bl ? bl->size() : 0, ci.groups);
    }
    sf.index.push_back(std::move(ci));
  }
  return ORCGPU_OK;
}

// One RowIndexEntry's positions dealt out to the column's streams (ORC specification, "Column encodings": the streams of a
// column record, in the order PRESENT, DATA, LENGTH | SECONDARY, {chunk header offset, bytes into the decompressed chunk} --
// uncompressed files {byte offset} --, run-length streams then {values of the current run consumed}, bit streams then
// {bits of the current byte consumed}).  false: the entry is not what such a column records.
struct EntrySplit {
  orcgpu_stream_entry present, data, second;  // second: LENGTH or SECONDARY
  bool has_data = false, has_second = false;
  int second_kind = 0;
};
bool split_index_entry(int orc_type, int encoding, bool has_present, bool compressed, const uint64_t* pos, uint32_t n, EntrySplit& out) {
  // per stream: 0 = none, 1 = bytes (no run), 2 = run-length values, 3 = bits over byte runs
  int data = 0, second = 0, second_kind = 0;
  const bool dict = encoding == ORCGPU_ENC_DICTIONARY || encoding == ORCGPU_ENC_DICTIONARY_V2;
  switch (orc_type) {
    case ORCGPU_T_BOOLEAN: data = 3; break;
    case ORCGPU_T_BYTE: case ORCGPU_T_SHORT: case ORCGPU_T_INT: case ORCGPU_T_LONG: case ORCGPU_T_DATE: data = 2; break;
    case ORCGPU_T_FLOAT: case ORCGPU_T_DOUBLE: data = 1; break;
    case ORCGPU_T_STRING: case ORCGPU_T_VARCHAR: case ORCGPU_T_CHAR:
      if (dict) data = 2;
      else data = 1, second = 2, second_kind = ORCGPU_S_LENGTH;
      break;
    case ORCGPU_T_BINARY: data = 1, second = 2, second_kind = ORCGPU_S_LENGTH; break;
    case ORCGPU_T_DECIMAL: data = 1, second = 2, second_kind = ORCGPU_S_SECONDARY; break;
    case ORCGPU_T_TIMESTAMP: case ORCGPU_T_TIMESTAMP_INSTANT: data = 2, second = 2, second_kind = ORCGPU_S_SECONDARY; break;
    case ORCGPU_T_LIST: case ORCGPU_T_MAP: second = 2, second_kind = ORCGPU_S_LENGTH; break;
    case ORCGPU_T_STRUCT: break;
    case ORCGPU_T_UNION: data = 2; break;
    default: return false;
  }
  uint32_t at = 0;
  bool ok = true;
  auto take = [&](int form, orcgpu_stream_entry& e) {
    e = orcgpu_stream_entry{0, 0, 0, 0};
    const uint32_t need = (compressed ? 2u : 1u) + (form >= 2 ? 1u : 0u) + (form == 3 ? 1u : 0u);
    if (at + need > n) {
      ok = false;
      return;
    }
    e.chunk_offset = pos[at++];
    uint64_t bytes = compressed ? pos[at++] : 0, values = form >= 2 ? pos[at++] : 0, bits = form == 3 ? pos[at++] : 0;
    if (bytes > 0xffffffffull || values > 0xffffffffull || bits > 7) ok = false;
    e.skip_bytes = (uint32_t)bytes;
    e.skip_values = (uint32_t)values;
    e.skip_bits = (uint32_t)bits;
  };
  if (has_present) take(3, out.present);
  out.has_data = data != 0;
  out.has_second = second != 0;
  out.second_kind = second_kind;
  if (data) take(data, out.data);
  if (second) take(second, out.second);
  return ok && at == n;
}

bool is_flat_kind(int k) {
  switch (k) {
    case ORCGPU_T_LIST: case ORCGPU_T_MAP: case ORCGPU_T_STRUCT: case ORCGPU_T_UNION: return false;
    default: return k >= 0 && k <= 18;
  }
}

// Estimated Arrow bytes per row of a column (what the column shard balances)
constexpr int kMetaMaxTypeDepth = 256;  // (stack safety only: the type list has been checked to be a tree)
double type_weight(const std::vector<OrcType>& types, uint32_t id, int depth = 0) {
  if (id >= types.size() || depth > kMetaMaxTypeDepth) return 0.0;
  const OrcType& t = types[id];
  double kids = 0.0;
  for (uint32_t k : t.subtypes) kids += type_weight(types, k, depth + 1);
  switch (t.kind) {
    case ORCGPU_T_BOOLEAN: return 0.125;
    case ORCGPU_T_BYTE: return 1;
    case ORCGPU_T_SHORT: return 2;
    case ORCGPU_T_INT: case ORCGPU_T_FLOAT: case ORCGPU_T_DATE: return 4;
    case ORCGPU_T_LONG: case ORCGPU_T_DOUBLE: case ORCGPU_T_TIMESTAMP: case ORCGPU_T_TIMESTAMP_INSTANT: return 8;
    case ORCGPU_T_DECIMAL: return 16;
    case ORCGPU_T_STRING: case ORCGPU_T_VARCHAR: case ORCGPU_T_CHAR: case ORCGPU_T_BINARY: return 4 + 16;
    case ORCGPU_T_STRUCT: return 0.125 + kids;
    case ORCGPU_T_UNION: return 1 + kids;
    case ORCGPU_T_LIST: case ORCGPU_T_MAP: return 4 + 2 * kids;
    default: return 8;
  }
}
// Longest-processing-time deal: items by falling weight (ties: the earlier first), each to the least loaded rank (ties: the lower)
void lpt_deal(const double* w, uint32_t n, uint32_t world, uint32_t* rank_of) {
  std::vector<uint32_t> order(n);
  for (uint32_t i = 0; i < n; i++) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return w[a] > w[b]; });
  std::vector<double> load(world ? world : 1, 0.0);
  for (uint32_t i : order) {
    uint32_t best = 0;
    for (uint32_t r = 1; r < load.size(); r++)
      if (load[r] < load[best]) best = r;
    rank_of[i] = best;
    load[best] += w[i];
  }
}

}  // namespace orcgpu_host
