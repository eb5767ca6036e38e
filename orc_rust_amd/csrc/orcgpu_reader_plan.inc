// orcgpu_reader_plan.inc -- what the file reader works out on the host with plain arithmetic, PURE C++ (no HIP, no device, no
// context, no reader handle): which columns a projection reads (ProjectionMask, with_schema's hints, the column shard), which
// stripes a rank owns, what of a stripe is staged under a predicate and a row selection (whole, or one piece per run of row
// groups), where a piece of a stream starts and ends, the orcgpu_column list of a stripe, and when staged pieces are grouped into
// one decode call.  Errors come back in a MetaErr as in orcgpu_meta.inc; the caller passes them on.
//
// Included by orcgpu_reader.inc (the product: liborcgpu.so) AND by tests/hostcheck/reader_plan_check.cpp, which compiles exactly
// this text with g++ -fsanitize=address,undefined and compares it with the blocks it was taken from
// (tests/test_reader_plan_sanitized.py).  The includer declares SelBatch (device/select_kernels.hip) in front of it.
#pragma once
#include <functional>

#include "orcgpu_meta.inc"
#include "orcgpu_selection.inc"
namespace orcgpu_host {

inline bool is_nested_kind(int k) { return k == ORCGPU_T_STRUCT || k == ORCGPU_T_LIST || k == ORCGPU_T_MAP || k == ORCGPU_T_UNION; }
// A string column whose values are indices into the stripe's dictionary (its LENGTH and DICTIONARY_DATA streams are the dictionary's)
inline bool is_string_dict_column(int kind, int encoding) {
  return (kind == ORCGPU_T_STRING || kind == ORCGPU_T_VARCHAR || kind == ORCGPU_T_CHAR) &&
         (encoding == ORCGPU_ENC_DICTIONARY || encoding == ORCGPU_ENC_DICTIONARY_V2);
}

// Arrow C Data Interface format string of a field -> ORCGPU_ARROW_* (+ precision / scale)
inline int arrow_code_of_format(const char* f, uint32_t* prec, uint32_t* scale) {
  *prec = *scale = 0;
  if (!f) return ORCGPU_ARROW_OTHER;
  const std::string s(f);
  if (s == "b") return ORCGPU_ARROW_BOOLEAN;
  if (s == "c") return ORCGPU_ARROW_INT8;
  if (s == "s") return ORCGPU_ARROW_INT16;
  if (s == "i") return ORCGPU_ARROW_INT32;
  if (s == "l") return ORCGPU_ARROW_INT64;
  if (s == "f") return ORCGPU_ARROW_FLOAT32;
  if (s == "g") return ORCGPU_ARROW_FLOAT64;
  if (s == "u") return ORCGPU_ARROW_UTF8;
  if (s == "z") return ORCGPU_ARROW_BINARY;
  if (s == "tdD") return ORCGPU_ARROW_DATE32;
  if (s.rfind("d:", 0) == 0) {
    int p = 0, sc = 0, bits = 128;
    if (sscanf(s.c_str(), "d:%d,%d,%d", &p, &sc, &bits) >= 2 && bits == 128 && p > 0) {
      *prec = (uint32_t)p;
      *scale = (uint32_t)sc;
      return ORCGPU_ARROW_DECIMAL128;
    }
    return ORCGPU_ARROW_OTHER;
  }
  if (s.size() >= 4 && s[0] == 't' && s[1] == 's' && s[3] == ':') {
    const int unit = s[2] == 's' ? 0 : (s[2] == 'm' ? 1 : (s[2] == 'u' ? 2 : (s[2] == 'n' ? 3 : -1)));
    if (unit < 0) return ORCGPU_ARROW_OTHER;
    const std::string tz = s.substr(4);
    if (tz.empty()) return ORCGPU_ARROW_TIMESTAMP_S_NOTZ + unit;
    if (tz == "UTC") return ORCGPU_ARROW_TIMESTAMP_S_UTC + unit;
    return ORCGPU_ARROW_TIMESTAMP_OTHER_TZ;
  }
  return ORCGPU_ARROW_OTHER;
}

// ---- the projection ---------------------------------------------------------------------------------------

// with_schema's fields as a tree (nested columns take nested hints: array_decoder/mod.rs:464-505)
struct SchemaNode {
  std::string format, name;
  int64_t flags = 0;
  std::vector<SchemaNode> kids;
};

// What the builder was told about the columns to read
struct ProjectionOptions {
  bool project_all = true;
  std::vector<std::string> projected_names;   // ProjectionMask::named_roots
  bool by_index = false;                      // ProjectionMask::roots
  std::vector<uint32_t> projected_roots;
  bool has_schema = false;                    // with_schema: per projected column, in order
  std::vector<SchemaNode> schema_tree;
  uint32_t shard_rank = 0, shard_world = 1;   // orcgpu_reader_set_shard
  int shard_mode = ORCGPU_SHARD_STRIPES;
  std::vector<std::string> dict_names;        // orcgpu_reader_set_dictionary_columns: root columns (file names) read as Dictionary(Int32, Utf8)
  int ts_arrow_target = ORCGPU_ARROW_TIMESTAMP_NS;
};

// One projected column: a root, or below a nested column one of its children (pre-order)
struct ProjCol {
  uint32_t id = 0;               // its type in the file's type list
  uint32_t parent = 0;           // 1 + index in Projection::cols of the column it is a child of (0: a root)
  std::string field;             // its field name there
  int target = 0;                // what with_schema's tree says about it: ORCGPU_ARROW_*
  uint32_t precision = 0, scale = 0;
  bool dict = false;             // read as a dictionary column
  uint32_t root = 0;             // index in Projection::names of the root column it is, or lies below
};
struct Projection {
  std::vector<ProjCol> cols;
  std::vector<std::string> names;  // of the projected ROOT columns
  // indices in `cols` of the root columns, in order: roots()[i] is the column named names[i]
  std::vector<size_t> roots() const {
    std::vector<size_t> out;
    for (size_t k = 0; k < cols.size(); k++)
      if (!cols[k].parent) out.push_back(k);
    return out;
  }
  std::vector<uint32_t> ids() const {
    std::vector<uint32_t> out;
    for (auto& c : cols) out.push_back(c.id);
    return out;
  }
  bool reads(uint32_t column_id) const {
    for (auto& c : cols)
      if (c.id == column_id) return true;
    return false;
  }
};

// The shard rule: with stripe shards, stripe number `at` of the reader's stripes belongs to rank at % world
inline bool stripe_is_mine(const ProjectionOptions& o, size_t at) {
  return !(o.shard_world > 1 && o.shard_mode == ORCGPU_SHARD_STRIPES && at % o.shard_world != o.shard_rank);
}

// The Arrow field with_schema gives for a column against the column's type: the target, and the fields its children are handed
// (zipped by position: struct_decoder.rs:43-48, list.rs, map.rs, union.rs).  A pair that does not match is ORCGPU_ARROW_OTHER,
// reported when the first stripe is planned, as MismatchedSchema.
inline int match_hint(const OrcType& t, const SchemaNode& hint, uint32_t* hp, uint32_t* hs, std::vector<const SchemaNode*>& kid_hints) {
  const std::string& f = hint.format;
  int target;
  if (!is_nested_kind(t.kind)) target = arrow_code_of_format(f.c_str(), hp, hs);
  else if (t.kind == ORCGPU_T_STRUCT && f == "+s" && hint.kids.size() == t.subtypes.size()) target = ORCGPU_ARROW_STRUCT;
  else if (t.kind == ORCGPU_T_LIST && f == "+l" && hint.kids.size() == 1) target = ORCGPU_ARROW_LIST;
  else if (t.kind == ORCGPU_T_MAP && f == "+m" && hint.kids.size() == 1 && hint.kids[0].format == "+s" && hint.kids[0].kids.size() == 2)
    target = (hint.flags & 4) ? ORCGPU_ARROW_MAP_SORTED : ORCGPU_ARROW_MAP;  // ARROW_FLAG_MAP_KEYS_SORTED
  else if (t.kind == ORCGPU_T_UNION && (f.rfind("+us:", 0) == 0 || f.rfind("+ud:", 0) == 0) && hint.kids.size() == t.subtypes.size()) target = ORCGPU_ARROW_UNION;
  else target = ORCGPU_ARROW_OTHER;
  if (target == ORCGPU_ARROW_STRUCT || target == ORCGPU_ARROW_UNION)
    for (size_t k = 0; k < kid_hints.size(); k++) kid_hints[k] = &hint.kids[k];
  else if (target == ORCGPU_ARROW_LIST) kid_hints[0] = &hint.kids[0];
  else if (target == ORCGPU_ARROW_MAP || target == ORCGPU_ARROW_MAP_SORTED) kid_hints[0] = &hint.kids[0].kids[0], kid_hints[1] = &hint.kids[0].kids[1];
  return target;
}

struct ProjectionWalk {
  const FileMetadata& md;
  const ProjectionOptions& o;
  Projection& out;
  MetaErr& err;
  const std::string& name;  // of the root column being walked (the file's)
  bool root_is_dict = false;
};
// A column and what lies below it: flat columns, and nested ones to any depth the decoder takes.  `hint`: the Arrow field
// with_schema gives for this column (nullptr: none)
inline int add_projected(ProjectionWalk& w, uint32_t id, uint32_t parent, const std::string& field, int depth, const SchemaNode* hint) {
  if (id >= w.md.types.size() || depth > kMetaMaxTypeDepth) return ORCGPU_OUT_OF_SPEC;  // (a type tree cannot be deeper than it has types: a cycle)
  const OrcType& t = w.md.types[id];
  const bool nested = is_nested_kind(t.kind);
  if (!nested && !is_flat_kind(t.kind)) {
    w.err.set("column '%s': ORC type kind %d is not decoded on the GPU path", w.name.c_str(), t.kind);
    return ORCGPU_UNSUPPORTED;
  }
  if ((t.kind == ORCGPU_T_LIST && t.subtypes.size() != 1) || (t.kind == ORCGPU_T_MAP && t.subtypes.size() != 2)) return ORCGPU_OUT_OF_SPEC;
  ProjCol c;
  c.id = id;
  c.parent = parent;
  c.field = hint && depth > 0 ? hint->name : field;
  c.root = (uint32_t)w.out.names.size() - 1;
  std::vector<const SchemaNode*> kid_hints(t.subtypes.size(), nullptr);
  if (hint) c.target = match_hint(t, *hint, &c.precision, &c.scale, kid_hints);
  c.dict = depth == 0 && std::find(w.o.dict_names.begin(), w.o.dict_names.end(), w.name) != w.o.dict_names.end();
  if (c.dict) w.root_is_dict = true;
  const int target = c.target;
  w.out.cols.push_back(std::move(c));
  const uint32_t me = (uint32_t)w.out.cols.size();
  if (nested && (!hint || target != ORCGPU_ARROW_OTHER))
    for (size_t f = 0; f < t.subtypes.size(); f++) {
      int rc = add_projected(w, t.subtypes[f], me, f < t.field_names.size() ? t.field_names[f] : std::string(), depth + 1, kid_hints[f]);
      if (rc) return rc;
    }
  return ORCGPU_OK;
}

// The root columns of the file this rank reads, as positions in the root type's subtypes; `pos_out`: each one's position among
// the projected columns of all ranks (the schema's field of the same position)
inline std::vector<size_t> roots_to_read(const FileMetadata& md, const ProjectionOptions& o, std::vector<size_t>& pos_out) {
  const OrcType& root = md.types[0];
  // the projected root columns, in file order; with_schema: columns and fields are zipped (array_decoder/mod.rs:577-582): columns
  // beyond the schema's fields are not decoded
  std::vector<size_t> taken;
  for (size_t k = 0; k < root.subtypes.size(); k++) {
    const std::string nm = k < root.field_names.size() ? root.field_names[k] : std::string();
    const bool take = o.project_all || (o.by_index ? std::find(o.projected_roots.begin(), o.projected_roots.end(), (uint32_t)k) != o.projected_roots.end()
                                                   : std::find(o.projected_names.begin(), o.projected_names.end(), nm) != o.projected_names.end());
    if (!take) continue;
    if (o.has_schema && taken.size() >= o.schema_tree.size()) break;
    taken.push_back(k);
  }
  // a column shard keeps this rank's share of them (orcgpu_reader_set_shard)
  std::vector<uint32_t> owner(taken.size(), o.shard_rank);
  if (o.shard_world > 1 && o.shard_mode == ORCGPU_SHARD_COLUMNS && !taken.empty()) {
    std::vector<double> w(taken.size());
    for (size_t i = 0; i < taken.size(); i++) w[i] = type_weight(md.types, root.subtypes[taken[i]]);
    lpt_deal(w.data(), (uint32_t)w.size(), o.shard_world, owner.data());
  }
  std::vector<size_t> mine;
  pos_out.clear();
  for (size_t ti = 0; ti < taken.size(); ti++)
    if (owner[ti] == o.shard_rank) {
      mine.push_back(taken[ti]);
      pos_out.push_back(ti);
    }
  return mine;
}

// ProjectionMask + with_schema + the column shard against the file's types -> the columns to read.  On an error `out` holds the
// columns walked so far.
inline int build_projection(const FileMetadata& md, const ProjectionOptions& o, Projection& out, MetaErr& err) {
  out.cols.clear();
  out.names.clear();
  if (md.types.empty()) return ORCGPU_OK;
  const OrcType& root = md.types[0];
  std::vector<std::string> dict_seen;  // the dictionary columns (orcgpu_reader_set_dictionary_columns) met among the columns read
  std::vector<size_t> pos;
  const std::vector<size_t> mine = roots_to_read(md, o, pos);
  for (size_t i = 0; i < mine.size(); i++) {
    const size_t k = mine[i];
    const std::string name = k < root.field_names.size() ? root.field_names[k] : std::string();
    const uint32_t cid = root.subtypes[k];
    if (cid >= md.types.size()) return ORCGPU_OUT_OF_SPEC;
    out.names.push_back(o.has_schema ? o.schema_tree[pos[i]].name : name);
    ProjectionWalk w{md, o, out, err, name};
    const int rc = add_projected(w, cid, 0, std::string(), 0, o.has_schema ? &o.schema_tree[pos[i]] : nullptr);
    if (w.root_is_dict) dict_seen.push_back(name);
    if (rc) return rc;
  }
  // (every dictionary column must be among the columns read)
  for (auto& dn : o.dict_names)
    if (std::find(dict_seen.begin(), dict_seen.end(), dn) == dict_seen.end() && o.shard_mode != ORCGPU_SHARD_COLUMNS) {
      err.set("dictionary column '%s' is not among the projected columns", dn.c_str());
      return ORCGPU_INVALID_ARGUMENT;
    }
  return ORCGPU_OK;
}

// The orcgpu_column list of a stripe: the projected columns as the file's types, the stripe's encodings and the builder describe them
inline std::vector<orcgpu_column> stripe_columns(const FileMetadata& md, const StripeFooter& sf, const Projection& proj, const ProjectionOptions& o) {
  std::vector<orcgpu_column> cols;
  for (const ProjCol& pc : proj.cols) {
    const uint32_t cid = pc.id;
    const OrcType& t = md.types[cid];
    orcgpu_column c{};
    c.column_id = cid;
    c.orc_type = t.kind;
    c.encoding = cid < sf.encodings.size() ? sf.encodings[cid].first : 0;
    c.dictionary_size = cid < sf.encodings.size() ? sf.encodings[cid].second : 0;
    c.precision = t.precision;
    c.scale = t.scale;
    c.arrow_target = (t.kind == ORCGPU_T_TIMESTAMP || t.kind == ORCGPU_T_TIMESTAMP_INSTANT) ? o.ts_arrow_target : 0;
    c.parent = pc.parent;
    if (o.has_schema) {
      c.arrow_target = pc.target;
      c.arrow_precision = pc.precision;
      c.arrow_scale = pc.scale;
    }
    // (dictionary output: with_schema's field for such a column is Utf8, or there is no schema; any other field stays and mismatches)
    if (pc.dict && (c.arrow_target == ORCGPU_ARROW_DEFAULT || c.arrow_target == ORCGPU_ARROW_UTF8)) c.arrow_target = ORCGPU_ARROW_DICTIONARY_UTF8;
    cols.push_back(c);
  }
  return cols;
}

// ---- pieces of streams ------------------------------------------------------------------------------------

// One stream of a stripe as it is read from the file: all of it, or from a row group's entry point on
struct StreamPiece {
  const StreamInfo* info;
  uint64_t start = 0, end = 0;  // bytes of the stream
  uint32_t skip_bytes = 0, skip_values = 0, skip_bits = 0;
  std::vector<orcgpu_stream_entry> entries;  // a whole stream: where its later row groups start, run starts for the walk (whole_stripe_entries)
};

inline bool is_data_stream(const Projection& proj, const StreamInfo& s) {
  if (!proj.reads(s.column)) return false;
  return !(s.kind == ORCGPU_S_ROW_INDEX || s.kind == ORCGPU_S_BLOOM_FILTER || s.kind == ORCGPU_S_BLOOM_FILTER_UTF8 || s.kind == ORCGPU_S_DICTIONARY_COUNT);
}

// Every data stream of the projected columns, whole
inline std::vector<StreamPiece> whole_stripe_pieces(const StripeFooter& sf, const Projection& proj) {
  std::vector<StreamPiece> whole;
  for (auto& s : sf.streams)
    if (is_data_stream(proj, s)) {
      StreamPiece pc;
      pc.info = &s;
      pc.end = s.length;
      whole.push_back(pc);
    }
  return whole;
}

// The entry of the stream of `kind` out of a RowIndexEntry dealt out to its column's streams.  false: a stream without positions
// (dictionaries), or one the column does not have
inline bool stream_entry(const EntrySplit& sp, int kind, bool has_present, orcgpu_stream_entry& e) {
  if (kind == ORCGPU_S_PRESENT && has_present) e = sp.present;
  else if (kind == ORCGPU_S_DATA && sp.has_data) e = sp.data;
  else if (sp.has_second && kind == sp.second_kind) e = sp.second;
  else return false;
  return true;
}

// A stream's column in a stripe whose ROW_INDEX streams have been read: its type and encoding, its index, whether it has a PRESENT stream
struct StreamColumn {
  const OrcType* type = nullptr;
  int encoding = 0;
  const ColumnIndex* index = nullptr;
  bool has_present = false;
  bool compressed = false;
  // RowIndexEntry `g` of the column -> the entry of the stream of `kind`
  bool entry(uint64_t g, int kind, orcgpu_stream_entry& e) const {
    EntrySplit sp;
    if (!split_index_entry(type->kind, encoding, has_present, compressed, index->positions.data() + g * index->per_group, index->per_group, sp)) return false;
    return stream_entry(sp, kind, has_present, e);
  }
};
inline StreamColumn stream_column(const FileMetadata& md, const StripeFooter& sf, const StreamInfo& s) {
  StreamColumn c;
  c.type = &md.types[s.column];
  c.encoding = s.column < sf.encodings.size() ? sf.encodings[s.column].first : 0;
  c.compressed = md.compression != ORCGPU_COMP_NONE;
  return c;
}
// ... and its index: false when the stripe has none for the column that holds n_groups entries of one length
inline bool stream_column_index(const StripeFooter& sf, const StreamInfo& s, uint64_t n_groups, StreamColumn& c) {
  for (auto& x : sf.index)
    if (x.column == s.column) c.index = &x;
  if (!c.index || !c.index->per_group || c.index->n_groups != n_groups) return false;
  for (auto& o : sf.streams) c.has_present = c.has_present || (o.column == s.column && o.kind == ORCGPU_S_PRESENT);
  return true;
}

// Where a piece that ends at the entry point `end` of the next row group really ends: a little beyond (the run, or the chunks,
// that straddle the boundary)
inline bool piece_end(const StreamInfo& s, bool compressed, ChunkReader& r, uint64_t& end) {
  if (!compressed) {
    end = std::min<uint64_t>(s.length, end + 8192);  // (the longest run: 512 values of 8 bytes, its header and patch list)
    return true;
  }
  // the chunk the boundary lies in and the one behind it (a run may straddle two chunks; a writer's chunks are full blocks but
  // for the last of a stream): their 3-byte headers say where they end
  for (int k = 0; k < 2 && end < s.length; k++) {
    std::vector<uint8_t> h;
    if (s.length - end < 3 || !r.get_bytes(s.offset + end, 3, h)) return false;
    const uint64_t len = ((uint64_t)h[0] | ((uint64_t)h[1] << 8) | ((uint64_t)h[2] << 16)) >> 1;
    if (len > s.length - end - 3) return false;
    end += 3 + len;
  }
  return true;
}

// The row groups [g0, g1) of a stripe as stream pieces: every stream from the entry point its column's RowIndexEntry g0 names
// to where entry g1 points (and a little beyond: piece_end).  false: the stripe's indexes cannot be used that way -- it is then
// decoded whole.
// (List / Map: their LENGTH stream is entered like any RLE stream, and their elements' streams at the positions the
// elements' own index entries hold for the same row group -- how many elements a piece has follows from its lengths, as in a
// whole stripe.  A Union: its tags -- byte RLE -- are entered like any run-length stream, and every arm's child at the
// positions the CHILD's own index entries hold for the row group: a writer records, at every row-group boundary, how far each
// column's streams have got, an arm's child included -- its count is the rows whose tag named it so far.  How many values of
// an arm a piece holds follows from the piece's tags, as in a whole stripe (union.rs:69-136).)
inline bool row_group_pieces(const FileMetadata& md, const StripeFooter& sf, const Projection& proj, ChunkReader& r, uint64_t n_groups, uint64_t g0,
                             uint64_t g1, std::vector<StreamPiece>& out) {
  out.clear();
  for (auto& s : sf.streams) {
    if (!is_data_stream(proj, s)) continue;
    StreamPiece pc;
    pc.info = &s;
    pc.end = s.length;
    StreamColumn col = stream_column(md, sf, s);
    if (s.kind == ORCGPU_S_DICTIONARY_DATA || (is_string_dict_column(col.type->kind, col.encoding) && s.kind == ORCGPU_S_LENGTH)) {  // dictionaries: whole
      out.push_back(pc);
      continue;
    }
    if (!stream_column_index(sf, s, n_groups, col)) return false;
    // a run holds at most 512 values; a chunk at most block_size bytes; a bit stream may be entered in mid-byte
    auto entry = [&](uint64_t g, orcgpu_stream_entry& e) {
      return col.entry(g, s.kind, e) && e.skip_bits <= 7 && e.skip_values <= 512 && e.skip_bytes <= md.block_size && e.chunk_offset <= s.length;
    };
    orcgpu_stream_entry e0{};
    if (!entry(g0, e0)) return false;
    pc.start = e0.chunk_offset;
    pc.skip_bytes = col.compressed ? e0.skip_bytes : 0;
    pc.skip_values = e0.skip_values;
    pc.skip_bits = e0.skip_bits;
    if (!col.compressed && e0.skip_bytes) return false;
    if (g1 < n_groups) {
      orcgpu_stream_entry e1{};
      if (!entry(g1, e1) || e1.chunk_offset < e0.chunk_offset) return false;
      pc.end = e1.chunk_offset;
      if (!piece_end(s, col.compressed, r, pc.end)) return false;
    }
    if (pc.start > pc.end) return false;
    out.push_back(pc);
  }
  return true;
}

// A stripe decoded whole whose ROW_INDEX streams have been read anyway (a predicate, a selection that needs all of it): the
// positions of its row groups go with the streams as verified run starts (orcgpu_stream::entries).  (Not with the pieces staged
// for a few row groups: a lane per entry follows its runs one global-memory round trip at a time, ~1 us each -- that pays for
// streams of long irregular runs, whose headers nothing else finds, not for some thousand short runs: a pruned read's walk went
// 0.7 -> 4.5 ms with them.)
constexpr uint64_t kEntriesMinBytesPerGroup = 16384;
inline void whole_stripe_entries(const FileMetadata& md, const StripeFooter& sf, uint64_t n_groups, std::vector<StreamPiece>& whole) {
  if (sf.index.empty() || n_groups < 2) return;
  for (auto& pc : whole) {
    const StreamInfo& s = *pc.info;
    if (s.column >= md.types.size()) continue;
    StreamColumn col = stream_column(md, sf, s);
    if (s.kind == ORCGPU_S_DICTIONARY_DATA || is_nested_kind(col.type->kind)) continue;
    if (is_string_dict_column(col.type->kind, col.encoding) && s.kind == ORCGPU_S_LENGTH) continue;
    // (a lane per entry follows its row group's runs one memory round trip at a time: worth it where the runs are long -- streams
    // of 16 KiB or more per row group --, not for the thousands of short runs of a narrow stream, which the span walk finds
    // faster by itself: with the positions of every stream a 24 M-row lineitem file read 8 ms slower)
    if (s.length / n_groups < kEntriesMinBytesPerGroup) continue;
    if (!stream_column_index(sf, s, n_groups, col)) continue;
    for (uint64_t g = 1; g < n_groups; g++) {
      orcgpu_stream_entry e{};
      if (!col.entry(g, s.kind, e) || e.skip_bytes > md.block_size || e.chunk_offset > s.length) {
        pc.entries.clear();
        break;
      }
      pc.entries.push_back(e);
    }
  }
}

// ---- what of a stripe is staged ---------------------------------------------------------------------------

// What the builder and the stripe's turn say about one stripe
struct StripeAsk {
  uint64_t n_rows = 0, stride = 0;            // StripeInformation.numberOfRows, Footer.rowIndexStride
  uint32_t batch_size = 8192;
  bool prune = true, has_filter = false;
  bool has_predicate = false;                 // with_predicate: ...
  bool predicate_ok = false;                  // ... its evaluation against the stripe's row indexes succeeded, and ...
  const std::vector<uint8_t>* keep = nullptr; // ... kept these row groups (predicate_row_groups)
};
// One staging call: a whole stripe, or a run of its row groups
struct StagePiece {
  std::vector<StreamPiece> pieces;
  uint64_t n_rows = 0;
  bool has_sel = false;
  std::vector<SelBatch> sel;      // the selection's batches, as rows of this piece
  bool is_piece = false;          // some row groups of the stripe, not the stripe
  uint64_t groups = 0;            // row groups read with it
};
struct StagePlan {
  std::vector<StagePiece> stages;  // none: nothing of the stripe is selected, it is not read at all
  uint64_t groups_total = 0, groups_read = 0;
};

inline uint64_t stripe_row_groups(uint64_t n_rows, uint64_t stride) { return stride ? (n_rows + stride - 1) / stride : 1; }

// arrow_reader.rs:258-293: the predicate against the stripe's row indexes -> the row groups to keep -> a RowSelection
// (from_row_group_filter, row_selection.rs:348-392: rows_per_group rows per kept / skipped group, neighbours merged); an
// evaluation that fails selects every row
inline std::vector<RowSel> predicate_selection(bool ok, const std::vector<uint8_t>& keep, uint64_t n_rows, uint64_t stride) {
  std::vector<RowSel> mine;
  if (!ok) {
    mine.push_back(RowSel{n_rows, false});  // RowSelection::select_all
    return mine;
  }
  if (keep.empty()) mine.push_back(RowSel{n_rows, true});  // RowSelection::skip_all
  for (uint8_t k : keep) {
    if (!mine.empty() && mine.back().skip == !k) mine.back().row_count += stride;
    else mine.push_back(RowSel{stride, !k});
  }
  return mine;
}

// arrow_reader.rs:296-308: the predicate's selection and the stripe's share of the row selection, intersected, as the batches the
// stripe yields.  `share`: what sel_split_off gave the stripe of with_row_selection's selection (null: there is none, or none of
// it is left).  false: there is neither -- the stripe is read whole, in the batches it has anyway
inline bool stripe_selection(const StripeAsk& a, const std::vector<RowSel>* share, std::vector<SelBatch>& batches) {
  bool has_sel = false;
  std::vector<RowSel> mine;
  if (a.has_predicate) {
    static const std::vector<uint8_t> none;
    mine = predicate_selection(a.predicate_ok, a.keep ? *a.keep : none, a.n_rows, a.stride);
    has_sel = true;
  }
  if (share) {
    mine = has_sel ? sel_intersect(*share, mine, a.n_rows) : *share;
    has_sel = true;
  }
  batches.clear();
  if (has_sel) batches = sel_batches(mine, a.n_rows, a.batch_size);
  return has_sel;
}

// The runs of consecutive row groups [first, second) that hold rows of the batches
inline std::vector<std::pair<uint64_t, uint64_t>> group_ranges(const std::vector<SelBatch>& batches, uint64_t stride, uint64_t n_groups, bool has_filter) {
  std::vector<uint8_t> needed(n_groups, 0);
  for (auto& b : batches)
    for (uint64_t g = b.start / stride; g <= (b.start + b.len - 1) / stride && g < n_groups; g++) needed[g] = 1;
  std::vector<std::pair<uint64_t, uint64_t>> ranges;
  for (uint64_t g = 0; g < n_groups; g++)
    if (needed[g]) {
      if (!ranges.empty() && ranges.back().second == g) ranges.back().second = g + 1;
      else ranges.push_back({g, g + 1});
    }
  // (a row filter packs a stripe's kept rows into batches: the stripe stays ONE result -- one run of row groups, from the
  // first to the last one wanted; the selection's batches skip what lies between)
  if (has_filter && ranges.size() > 1) ranges = {{ranges.front().first, ranges.back().second}};
  return ranges;
}

// A selection that asks for every row in the batches the stripe has anyway -- a predicate that keeps all row groups -- is none
inline bool batches_as_decoded(const std::vector<SelBatch>& batches, uint64_t n_rows, uint32_t batch_size) {
  bool as_decoded = batch_size && batches.size() == (n_rows + batch_size - 1) / batch_size;
  for (size_t k = 0; k < batches.size() && as_decoded; k++)
    as_decoded = batches[k].start == (uint64_t)k * batch_size && batches[k].len == std::min<uint64_t>(batch_size, n_rows - batches[k].start);
  return as_decoded;
}

// The selected row groups of a stripe as one staging call per run of them, the batches re-based onto their piece.  false: the
// selection wants every row group, or the stripe's indexes cannot be used -- the stripe is decoded whole
inline bool plan_row_group_pieces(const FileMetadata& md, const StripeFooter& sf, const Projection& proj, ChunkReader& r, const StripeAsk& a,
                                  const std::vector<SelBatch>& batches, uint64_t n_groups, StagePlan& plan) {
  const std::vector<std::pair<uint64_t, uint64_t>> ranges = group_ranges(batches, a.stride, n_groups, a.has_filter);
  std::vector<std::vector<StreamPiece>> pieces(ranges.size());
  bool usable = !(ranges.size() == 1 && ranges[0].first == 0 && ranges[0].second == n_groups);
  for (size_t k = 0; k < ranges.size() && usable; k++) usable = row_group_pieces(md, sf, proj, r, n_groups, ranges[k].first, ranges[k].second, pieces[k]);
  if (!usable) return false;
  for (size_t k = 0; k < ranges.size(); k++) {
    const uint64_t r0 = ranges[k].first * a.stride, r1 = std::min<uint64_t>(a.n_rows, ranges[k].second * a.stride);
    StagePiece st;
    st.pieces = std::move(pieces[k]);
    st.n_rows = r1 - r0;
    st.has_sel = true;
    st.is_piece = true;
    for (auto& b : batches)
      if (b.start >= r0 && b.start < r1) st.sel.push_back(SelBatch{b.start - r0, b.len, 0});
    st.groups = ranges[k].second - ranges[k].first;
    plan.groups_read += st.groups;
    plan.stages.push_back(std::move(st));
  }
  return true;
}

// One stripe -> what is staged of it: the whole stripe, or -- under a selection, when its ROW_INDEX streams allow it -- one piece
// per run of consecutive row groups that hold selected rows (none: the stripe is not read at all).  `need_index` is called
// before the stripe's index is looked at for positions when sf.index_read is not set: it reads the index into sf (or leaves it
// empty: the stripe is then decoded whole).
inline StagePlan plan_stripe(const FileMetadata& md, const StripeFooter& sf, const Projection& proj, ChunkReader& r, const StripeAsk& a,
                             const std::vector<RowSel>* share, const std::function<void()>& need_index) {
  StagePlan plan;
  std::vector<SelBatch> batches;
  const bool has_sel = stripe_selection(a, share, batches);
  const uint64_t n_groups = stripe_row_groups(a.n_rows, a.stride);
  plan.groups_total = n_groups;
  if (has_sel && a.prune) {
    if (batches.empty()) return plan;  // nothing of the stripe is selected: not read
    if (a.stride && n_groups > 1) {
      if (!sf.index_read) need_index();
      if (plan_row_group_pieces(md, sf, proj, r, a, batches, n_groups, plan)) return plan;
    }
  }
  StagePiece st;
  st.pieces = whole_stripe_pieces(sf, proj);
  if (sf.index_read && a.stride) whole_stripe_entries(md, sf, n_groups, st.pieces);
  st.n_rows = a.n_rows;
  st.has_sel = has_sel && !batches_as_decoded(batches, a.n_rows, a.batch_size);
  if (st.has_sel) st.sel = std::move(batches);
  st.groups = n_groups;
  plan.groups_read = n_groups;
  plan.stages.push_back(std::move(st));
  return plan;
}

// ---- the grouping policy: a decode call costs its longest block chain (milliseconds) however little it decodes, so small
// pieces -- what a selection leaves of its stripes -- share one ----------------------------------------------
constexpr size_t kGroupMaxPieces = 32;               // staged pieces one decode call takes
constexpr uint64_t kGroupMaxBytes = 64u << 20;       // ... and their staged bytes
constexpr uint64_t kWakeBytesPieces = 48u << 20;     // staged bytes the decoder waits for while the stager is at work: pieces only ...
constexpr uint64_t kWakeBytesMixed = 8u << 20;       // ... and with a whole stripe among them

// The stager may stage more: it is less than 2 x prefetch stripes ahead of the decoder -- small pieces queue up beyond that, up to
// what one call takes.  (prefetch = 0: the serial path's "one more stripe into this call")
inline bool stager_has_room(size_t queued, uint64_t queued_bytes, uint32_t prefetch) {
  if (queued < 2 * (size_t)prefetch) return true;
  return queued < kGroupMaxPieces && queued_bytes < kGroupMaxBytes;
}
// The decoder should start a call while the stager is still at work: the queue holds what one call takes, or enough bytes
inline bool decoder_should_wake(size_t queued, uint64_t queued_bytes, bool pieces_only) {
  if (!queued) return false;
  return queued >= kGroupMaxPieces || queued_bytes >= (pieces_only ? kWakeBytesPieces : kWakeBytesMixed);
}
// The next staged piece joins the call's group: as many as the caller has room for -- and small pieces whatever the room
inline bool joins_group(size_t group_size, uint64_t group_bytes, uint64_t next_bytes, size_t room) {
  return group_size < kGroupMaxPieces && (group_size < room || group_bytes + next_bytes <= kGroupMaxBytes);
}

}  // namespace orcgpu_host
