// reader_plan_check.cpp -- the file reader's host planning (orc_rust_amd/csrc/orcgpu_reader_plan.inc, the very text
// liborcgpu.so is built from) under AddressSanitizer + UBSan on the CPU (TEST INFRASTRUCTURE; tests/test_reader_plan_sanitized.py).
//
// The planning file was taken out of one reader file whose blocks worked on the reader handle.  Those blocks are kept here as
// they were (ref_*: the projection walk of reader_build, the selection / ranges / as_decoded part of reader_stage_next,
// row_group_pieces, whole_stripe_entries, the orcgpu_column fill of reader_stage_rows, the three grouping conditions of the serial
// path, the stager and the decoder), on a plain struct in place of the handle, and compared field by field with what the planning
// file gives: over seeded random inputs and over the cases written out by hand below.  One line per case, then the count.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "../../include/orcgpu.h"
struct SelBatch {  // (device/select_kernels.hip: what the selection kernel takes per selected batch)
  uint64_t start;
  uint32_t len;
  uint32_t pad;
};
#include "../../orc_rust_amd/csrc/orcgpu_reader_plan.inc"

using namespace orcgpu_host;

// ---- the blocks as they stood in the reader file --------------------------------------------------------------------
constexpr int kMaxTypeDepth = 256;
struct RefReader {
  FileMetadata md;
  ChunkReader* reader = nullptr;
  uint32_t batch_size = 8192;
  bool project_all = true;
  std::vector<std::string> projected_names;
  int ts_arrow_target = ORCGPU_ARROW_TIMESTAMP_NS;
  std::vector<std::string> col_names;
  std::vector<uint32_t> col_ids, col_parent;
  std::vector<std::string> col_field;
  bool by_index = false;
  std::vector<uint32_t> projected_roots;
  bool has_schema = false;
  std::vector<int> schema_target;
  std::vector<std::string> schema_names;
  std::vector<SchemaNode> schema_tree;
  uint32_t shard_rank = 0, shard_world = 1;
  int shard_mode = ORCGPU_SHARD_STRIPES;
  std::vector<int> col_target;
  std::vector<uint32_t> col_precision, col_scale;
  std::vector<std::string> dict_names;
  std::vector<uint8_t> col_dict;
  bool prune = true, has_filter = false;
  char err[512] = {0};
};
static void ref_set_err(RefReader* rd, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
static void ref_set_err(RefReader* rd, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(rd->err, sizeof(rd->err), fmt, ap);
  va_end(ap);
}

static int ref_build(RefReader* rd) {
  rd->col_names.clear();
  rd->col_ids.clear();
  rd->col_parent.clear();
  rd->col_field.clear();
  rd->col_target.clear();
  rd->col_precision.clear();
  rd->col_scale.clear();
  rd->col_dict.clear();
  if (rd->md.types.empty()) return ORCGPU_OK;
  const OrcType& root = rd->md.types[0];
  std::vector<std::string> dict_seen;
  std::vector<size_t> taken;
  for (size_t k = 0; k < root.subtypes.size(); k++) {
    const std::string nm = k < root.field_names.size() ? root.field_names[k] : std::string();
    const bool take = rd->project_all || (rd->by_index ? std::find(rd->projected_roots.begin(), rd->projected_roots.end(), (uint32_t)k) != rd->projected_roots.end()
                                                       : std::find(rd->projected_names.begin(), rd->projected_names.end(), nm) != rd->projected_names.end());
    if (!take) continue;
    if (rd->has_schema && taken.size() >= rd->schema_target.size()) break;
    taken.push_back(k);
  }
  std::vector<uint32_t> owner(taken.size(), rd->shard_rank);
  if (rd->shard_world > 1 && rd->shard_mode == ORCGPU_SHARD_COLUMNS && !taken.empty()) {
    std::vector<double> w(taken.size());
    for (size_t i = 0; i < taken.size(); i++) w[i] = type_weight(rd->md.types, root.subtypes[taken[i]]);
    lpt_deal(w.data(), (uint32_t)w.size(), rd->shard_world, owner.data());
  }
  for (size_t ti = 0; ti < taken.size(); ti++) {
    if (owner[ti] != rd->shard_rank) continue;
    const size_t k = taken[ti];
    std::string name = k < root.field_names.size() ? root.field_names[k] : std::string();
    uint32_t cid = root.subtypes[k];
    if (cid >= rd->md.types.size()) return ORCGPU_OUT_OF_SPEC;
    std::function<int(uint32_t, uint32_t, const std::string&, int, const SchemaNode*)> add = [&](uint32_t id, uint32_t parent, const std::string& field, int depth,
                                                                                               const SchemaNode* hint) -> int {
      if (id >= rd->md.types.size() || depth > kMaxTypeDepth) return ORCGPU_OUT_OF_SPEC;
      const OrcType& t = rd->md.types[id];
      const bool nested = t.kind == ORCGPU_T_STRUCT || t.kind == ORCGPU_T_LIST || t.kind == ORCGPU_T_MAP || t.kind == ORCGPU_T_UNION;
      if (!nested && !is_flat_kind(t.kind)) {
        ref_set_err(rd, "column '%s': ORC type kind %d is not decoded on the GPU path", name.c_str(), t.kind);
        return ORCGPU_UNSUPPORTED;
      }
      if ((t.kind == ORCGPU_T_LIST && t.subtypes.size() != 1) || (t.kind == ORCGPU_T_MAP && t.subtypes.size() != 2)) return ORCGPU_OUT_OF_SPEC;
      rd->col_ids.push_back(id);
      rd->col_parent.push_back(parent);
      rd->col_field.push_back(hint && depth > 0 ? hint->name : field);
      uint32_t hp = 0, hs = 0;
      int target = 0;
      std::vector<const SchemaNode*> kid_hints(t.subtypes.size(), nullptr);
      if (hint) {
        const std::string& f = hint->format;
        if (!nested) target = arrow_code_of_format(f.c_str(), &hp, &hs);
        else if (t.kind == ORCGPU_T_STRUCT && f == "+s" && hint->kids.size() == t.subtypes.size()) target = ORCGPU_ARROW_STRUCT;
        else if (t.kind == ORCGPU_T_LIST && f == "+l" && hint->kids.size() == 1) target = ORCGPU_ARROW_LIST;
        else if (t.kind == ORCGPU_T_MAP && f == "+m" && hint->kids.size() == 1 && hint->kids[0].format == "+s" && hint->kids[0].kids.size() == 2)
          target = (hint->flags & 4) ? ORCGPU_ARROW_MAP_SORTED : ORCGPU_ARROW_MAP;
        else if (t.kind == ORCGPU_T_UNION && (f.rfind("+us:", 0) == 0 || f.rfind("+ud:", 0) == 0) && hint->kids.size() == t.subtypes.size()) target = ORCGPU_ARROW_UNION;
        else target = ORCGPU_ARROW_OTHER;
        if (target == ORCGPU_ARROW_STRUCT || target == ORCGPU_ARROW_UNION)
          for (size_t k = 0; k < kid_hints.size(); k++) kid_hints[k] = &hint->kids[k];
        else if (target == ORCGPU_ARROW_LIST) kid_hints[0] = &hint->kids[0];
        else if (target == ORCGPU_ARROW_MAP || target == ORCGPU_ARROW_MAP_SORTED) kid_hints[0] = &hint->kids[0].kids[0], kid_hints[1] = &hint->kids[0].kids[1];
      }
      rd->col_target.push_back(target);
      rd->col_precision.push_back(hp);
      rd->col_scale.push_back(hs);
      const bool as_dict = depth == 0 && std::find(rd->dict_names.begin(), rd->dict_names.end(), name) != rd->dict_names.end();
      rd->col_dict.push_back(as_dict ? 1 : 0);
      if (as_dict) dict_seen.push_back(name);
      const uint32_t me = (uint32_t)rd->col_ids.size();
      if (nested && (!hint || target != ORCGPU_ARROW_OTHER))
        for (size_t f = 0; f < t.subtypes.size(); f++) {
          int rc = add(t.subtypes[f], me, f < t.field_names.size() ? t.field_names[f] : std::string(), depth + 1, kid_hints[f]);
          if (rc) return rc;
        }
      return ORCGPU_OK;
    };
    const size_t root_pos = ti;
    rd->col_names.push_back(rd->has_schema ? rd->schema_names[root_pos] : name);
    int rc = add(cid, 0, std::string(), 0, rd->has_schema ? &rd->schema_tree[root_pos] : nullptr);
    if (rc) return rc;
  }
  for (auto& dn : rd->dict_names)
    if (std::find(dict_seen.begin(), dict_seen.end(), dn) == dict_seen.end() && rd->shard_mode != ORCGPU_SHARD_COLUMNS) {
      ref_set_err(rd, "dictionary column '%s' is not among the projected columns", dn.c_str());
      return ORCGPU_INVALID_ARGUMENT;
    }
  return ORCGPU_OK;
}

static std::vector<orcgpu_column> ref_columns(RefReader* rd, const StripeFooter& sf) {
  std::vector<orcgpu_column> cols;
  for (uint32_t cid : rd->col_ids) {
    const OrcType& t = rd->md.types[cid];
    orcgpu_column c{};
    c.column_id = cid;
    c.orc_type = t.kind;
    c.encoding = cid < sf.encodings.size() ? sf.encodings[cid].first : 0;
    c.dictionary_size = cid < sf.encodings.size() ? sf.encodings[cid].second : 0;
    c.precision = t.precision;
    c.scale = t.scale;
    c.arrow_target = (t.kind == ORCGPU_T_TIMESTAMP || t.kind == ORCGPU_T_TIMESTAMP_INSTANT) ? rd->ts_arrow_target : 0;
    c.parent = rd->col_parent[cols.size()];
    if (rd->has_schema) {
      const size_t k = cols.size();
      c.arrow_target = rd->col_target[k];
      c.arrow_precision = rd->col_precision[k];
      c.arrow_scale = rd->col_scale[k];
    }
    if (rd->col_dict[cols.size()] && (c.arrow_target == ORCGPU_ARROW_DEFAULT || c.arrow_target == ORCGPU_ARROW_UTF8)) c.arrow_target = ORCGPU_ARROW_DICTIONARY_UTF8;
    cols.push_back(c);
  }
  return cols;
}

static bool ref_is_data_stream(const RefReader* rd, const StreamInfo& s) {
  if (std::find(rd->col_ids.begin(), rd->col_ids.end(), s.column) == rd->col_ids.end()) return false;
  return !(s.kind == ORCGPU_S_ROW_INDEX || s.kind == ORCGPU_S_BLOOM_FILTER || s.kind == ORCGPU_S_BLOOM_FILTER_UTF8 || s.kind == ORCGPU_S_DICTIONARY_COUNT);
}

static bool ref_row_group_pieces(RefReader* rd, const StripeFooter& sf, uint64_t n_groups, uint64_t g0, uint64_t g1, std::vector<StreamPiece>& out) {
  const bool compressed = rd->md.compression != ORCGPU_COMP_NONE;
  out.clear();
  for (auto& s : sf.streams) {
    if (!ref_is_data_stream(rd, s)) continue;
    StreamPiece pc;
    pc.info = &s;
    pc.end = s.length;
    const OrcType& t = rd->md.types[s.column];
    const int enc = s.column < sf.encodings.size() ? sf.encodings[s.column].first : 0;
    const bool dict_col = (t.kind == ORCGPU_T_STRING || t.kind == ORCGPU_T_VARCHAR || t.kind == ORCGPU_T_CHAR) &&
                          (enc == ORCGPU_ENC_DICTIONARY || enc == ORCGPU_ENC_DICTIONARY_V2);
    if (s.kind == ORCGPU_S_DICTIONARY_DATA || (dict_col && s.kind == ORCGPU_S_LENGTH)) {
      out.push_back(pc);
      continue;
    }
    const ColumnIndex* ci = nullptr;
    for (auto& x : sf.index)
      if (x.column == s.column) ci = &x;
    if (!ci || !ci->per_group || ci->n_groups != n_groups) return false;
    bool has_present = false;
    for (auto& o : sf.streams) has_present = has_present || (o.column == s.column && o.kind == ORCGPU_S_PRESENT);
    auto entry = [&](uint64_t g, orcgpu_stream_entry& e) -> bool {
      EntrySplit sp;
      if (!split_index_entry(t.kind, enc, has_present, compressed, ci->positions.data() + g * ci->per_group, ci->per_group, sp)) return false;
      if (s.kind == ORCGPU_S_PRESENT && has_present) e = sp.present;
      else if (s.kind == ORCGPU_S_DATA && sp.has_data) e = sp.data;
      else if (sp.has_second && s.kind == sp.second_kind) e = sp.second;
      else return false;
      return e.skip_bits <= 7 && e.skip_values <= 512 && e.skip_bytes <= rd->md.block_size && e.chunk_offset <= s.length;
    };
    orcgpu_stream_entry e0{};
    if (!entry(g0, e0)) return false;
    pc.start = e0.chunk_offset;
    pc.skip_bytes = compressed ? e0.skip_bytes : 0;
    pc.skip_values = e0.skip_values;
    pc.skip_bits = e0.skip_bits;
    if (!compressed && e0.skip_bytes) return false;
    if (g1 < n_groups) {
      orcgpu_stream_entry e1{};
      if (!entry(g1, e1) || e1.chunk_offset < e0.chunk_offset) return false;
      uint64_t end = e1.chunk_offset;
      if (compressed) {
        for (int k = 0; k < 2 && end < s.length; k++) {
          std::vector<uint8_t> h;
          if (s.length - end < 3 || !rd->reader->get_bytes(s.offset + end, 3, h)) return false;
          const uint64_t len = ((uint64_t)h[0] | ((uint64_t)h[1] << 8) | ((uint64_t)h[2] << 16)) >> 1;
          if (len > s.length - end - 3) return false;
          end += 3 + len;
        }
      } else {
        end = std::min<uint64_t>(s.length, end + 8192);
      }
      pc.end = end;
    }
    if (pc.start > pc.end) return false;
    out.push_back(pc);
  }
  return true;
}

static void ref_whole_stripe_entries(RefReader* rd, const StripeFooter& sf, uint64_t n_groups, std::vector<StreamPiece>& whole) {
  const bool compressed = rd->md.compression != ORCGPU_COMP_NONE;
  if (sf.index.empty() || n_groups < 2) return;
  for (auto& pc : whole) {
    const StreamInfo& s = *pc.info;
    if (s.column >= rd->md.types.size()) continue;
    const OrcType& t = rd->md.types[s.column];
    const int enc = s.column < sf.encodings.size() ? sf.encodings[s.column].first : 0;
    if (s.kind == ORCGPU_S_DICTIONARY_DATA || t.kind == ORCGPU_T_LIST || t.kind == ORCGPU_T_MAP || t.kind == ORCGPU_T_UNION || t.kind == ORCGPU_T_STRUCT) continue;
    const bool dict_col = (t.kind == ORCGPU_T_STRING || t.kind == ORCGPU_T_VARCHAR || t.kind == ORCGPU_T_CHAR) &&
                          (enc == ORCGPU_ENC_DICTIONARY || enc == ORCGPU_ENC_DICTIONARY_V2);
    if (dict_col && s.kind == ORCGPU_S_LENGTH) continue;
    if (s.length / n_groups < 16384) continue;
    const ColumnIndex* ci = nullptr;
    for (auto& x : sf.index)
      if (x.column == s.column) ci = &x;
    if (!ci || !ci->per_group || ci->n_groups != n_groups) continue;
    bool has_present = false;
    for (auto& o : sf.streams) has_present = has_present || (o.column == s.column && o.kind == ORCGPU_S_PRESENT);
    for (uint64_t g = 1; g < n_groups; g++) {
      EntrySplit sp;
      orcgpu_stream_entry e{};
      bool ok = split_index_entry(t.kind, enc, has_present, compressed, ci->positions.data() + g * ci->per_group, ci->per_group, sp);
      if (ok && s.kind == ORCGPU_S_PRESENT && has_present) e = sp.present;
      else if (ok && s.kind == ORCGPU_S_DATA && sp.has_data) e = sp.data;
      else if (ok && sp.has_second && s.kind == sp.second_kind) e = sp.second;
      else ok = false;
      if (!ok || e.skip_bytes > rd->md.block_size || e.chunk_offset > s.length) {
        pc.entries.clear();
        break;
      }
      pc.entries.push_back(e);
    }
  }
}

// What reader_stage_next staged, in order (reader_stage_rows and the fields it set on the staged stripe, recorded)
struct RefStaged {
  std::vector<StreamPiece> pieces;
  uint64_t n_rows = 0;
  bool has_sel = false, piece = false;
  std::vector<SelBatch> sel;
};
struct RefPlan {
  std::vector<RefStaged> out;
  uint64_t groups_total = 0, groups_read = 0;
  int index_reads = 0;
};
// (has_predicate / pred_ok / keep: what predicate_row_groups gave; `selection`: what is left of the reader's row selection)
static void ref_stage_next(RefReader* rd, StripeFooter& sf, uint64_t n_rows, bool has_predicate, bool pred_ok, const std::vector<uint8_t>& keep, bool has_selection,
                           std::vector<RowSel>& selection, RefPlan& P) {
  bool has_sel = false;
  std::vector<SelBatch> batches;
  std::vector<RowSel> mine;
  const uint64_t stride = rd->md.row_index_stride;
  if (has_predicate) {
    if (pred_ok) {
      if (keep.empty()) mine.push_back(RowSel{n_rows, true});
      for (uint8_t k : keep) {
        if (!mine.empty() && mine.back().skip == !k) mine.back().row_count += stride;
        else mine.push_back(RowSel{stride, !k});
      }
    } else {
      mine.push_back(RowSel{n_rows, false});
    }
    has_sel = true;
  }
  if (has_selection && sel_row_count(selection) > 0) {
    std::vector<RowSel> share = sel_split_off(selection, n_rows);
    mine = has_sel ? sel_intersect(share, mine, n_rows) : share;
    has_sel = true;
  }
  if (has_sel) batches = sel_batches(mine, n_rows, rd->batch_size);
  const uint64_t n_groups = stride ? (n_rows + stride - 1) / stride : 1;
  P.groups_total += n_groups;
  std::vector<StreamPiece> whole;
  for (auto& s : sf.streams)
    if (ref_is_data_stream(rd, s)) {
      StreamPiece pc;
      pc.info = &s;
      pc.end = s.length;
      whole.push_back(pc);
    }
  if (has_sel && rd->prune) {
    if (batches.empty()) return;
    if (stride && n_groups > 1) {
      if (!sf.index_read) P.index_reads++;
      std::vector<uint8_t> needed(n_groups, 0);
      for (auto& b : batches)
        for (uint64_t g = b.start / stride; g <= (b.start + b.len - 1) / stride && g < n_groups; g++) needed[g] = 1;
      std::vector<std::pair<uint64_t, uint64_t>> ranges;
      for (uint64_t g = 0; g < n_groups; g++)
        if (needed[g]) {
          if (!ranges.empty() && ranges.back().second == g) ranges.back().second = g + 1;
          else ranges.push_back({g, g + 1});
        }
      if (rd->has_filter && ranges.size() > 1) ranges = {{ranges.front().first, ranges.back().second}};
      std::vector<std::vector<StreamPiece>> pieces(ranges.size());
      bool usable = !(ranges.size() == 1 && ranges[0].first == 0 && ranges[0].second == n_groups);
      for (size_t k = 0; k < ranges.size() && usable; k++) usable = ref_row_group_pieces(rd, sf, n_groups, ranges[k].first, ranges[k].second, pieces[k]);
      if (usable) {
        for (size_t k = 0; k < ranges.size(); k++) {
          const uint64_t r0 = ranges[k].first * stride, r1 = std::min<uint64_t>(n_rows, ranges[k].second * stride);
          RefStaged st;
          st.pieces = pieces[k];
          st.n_rows = r1 - r0;
          st.has_sel = true;
          st.piece = true;
          for (auto& b : batches)
            if (b.start >= r0 && b.start < r1) st.sel.push_back(SelBatch{b.start - r0, b.len, 0});
          P.groups_read += ranges[k].second - ranges[k].first;
          P.out.push_back(st);
        }
        return;
      }
    }
  }
  if (sf.index_read && stride) ref_whole_stripe_entries(rd, sf, n_groups, whole);
  RefStaged st;
  st.pieces = whole;
  st.n_rows = n_rows;
  bool as_decoded = has_sel && rd->batch_size && batches.size() == (n_rows + rd->batch_size - 1) / rd->batch_size;
  for (size_t k = 0; k < batches.size() && as_decoded; k++)
    as_decoded = batches[k].start == (uint64_t)k * rd->batch_size && batches[k].len == std::min<uint64_t>(rd->batch_size, n_rows - batches[k].start);
  st.has_sel = has_sel && !as_decoded;
  if (st.has_sel) st.sel = std::move(batches);
  P.groups_read += n_groups;
  P.out.push_back(st);
}

// the three grouping conditions: the serial path's "one more", the stager's wait, the decoder's wait and its group loop
static bool ref_serial_more(size_t got, uint64_t staged_bytes) { return got < 32 && staged_bytes < (64u << 20); }
static bool ref_stager_room(size_t queued, uint64_t bytes, uint32_t prefetch) {
  if (queued < 2 * (size_t)prefetch) return true;
  return queued < 32 && bytes < (64u << 20);
}
static bool ref_decoder_wake(size_t queued, uint64_t bytes, bool pieces_only) {
  if (queued == 0) return false;
  return queued >= 32 || bytes >= (pieces_only ? (48u << 20) : (8u << 20));
}
static bool ref_joins(size_t group, uint64_t group_bytes, uint64_t next, size_t room) { return group < 32 && (group < room || group_bytes + next <= (64u << 20)); }

// ---- comparing --------------------------------------------------------------------------------------------------------
static int g_cases = 0, g_mismatches = 0;
static void report(const char* name, size_t calls, size_t bad) {
  g_cases++;
  g_mismatches += bad != 0;
  if (bad) printf("%s: %zu calls: %zu DIFFER\n", name, calls, bad);
  else printf("%s: %zu calls: same\n", name, calls);
}

static ProjectionOptions options_of(const RefReader& R) {
  ProjectionOptions o;
  o.project_all = R.project_all;
  o.projected_names = R.projected_names;
  o.by_index = R.by_index;
  o.projected_roots = R.projected_roots;
  o.has_schema = R.has_schema;
  o.schema_tree = R.schema_tree;
  o.shard_rank = R.shard_rank;
  o.shard_world = R.shard_world;
  o.shard_mode = R.shard_mode;
  o.dict_names = R.dict_names;
  o.ts_arrow_target = R.ts_arrow_target;
  return o;
}
static void set_schema(RefReader& R, const std::vector<SchemaNode>& tree) {  // (orcgpu_reader_set_schema)
  R.has_schema = true;
  R.schema_tree = tree;
  R.schema_target.clear();
  R.schema_names.clear();
  for (auto& n : tree) {
    uint32_t p, s;
    R.schema_target.push_back(arrow_code_of_format(n.format.c_str(), &p, &s));
    R.schema_names.push_back(n.name);
  }
}

// the projection: rc, message, names, and every column's record against the parallel vectors (also after an error)
static bool same_projection(RefReader& R, int* rc_out = nullptr, Projection* proj_out = nullptr) {
  R.err[0] = 0;
  const int rc_ref = ref_build(&R);
  Projection P;
  MetaErr e;
  const int rc = build_projection(R.md, options_of(R), P, e);
  bool same = rc == rc_ref && !strcmp(e.msg, R.err) && P.names == R.col_names && P.cols.size() == R.col_ids.size() &&
              R.col_parent.size() == P.cols.size() && R.col_field.size() == P.cols.size() && R.col_target.size() == P.cols.size() &&
              R.col_precision.size() == P.cols.size() && R.col_scale.size() == P.cols.size() && R.col_dict.size() == P.cols.size();
  size_t root = 0;
  std::vector<size_t> roots;
  for (size_t k = 0; k < P.cols.size() && same; k++) {
    const ProjCol& c = P.cols[k];
    same = c.id == R.col_ids[k] && c.parent == R.col_parent[k] && c.field == R.col_field[k] && c.target == R.col_target[k] &&
           c.precision == R.col_precision[k] && c.scale == R.col_scale[k] && c.dict == (R.col_dict[k] != 0);
    if (!R.col_parent[k]) {  // (the walk over root columns as it was written out: `root` counts them)
      same = same && c.root == root;
      roots.push_back(k);
      root++;
    } else {
      same = same && c.root == root - 1;
    }
  }
  same = same && (roots == P.roots() || !same) && P.ids() == R.col_ids;
  if (rc_out) *rc_out = rc;
  if (proj_out) *proj_out = P;
  return same;
}

static bool same_pieces(const std::vector<StreamPiece>& a, const std::vector<StreamPiece>& b) {
  if (a.size() != b.size()) return false;
  for (size_t k = 0; k < a.size(); k++) {
    if (a[k].info != b[k].info || a[k].start != b[k].start || a[k].end != b[k].end || a[k].skip_bytes != b[k].skip_bytes ||
        a[k].skip_values != b[k].skip_values || a[k].skip_bits != b[k].skip_bits || a[k].entries.size() != b[k].entries.size())
      return false;
    for (size_t j = 0; j < a[k].entries.size(); j++) {
      const orcgpu_stream_entry &x = a[k].entries[j], &y = b[k].entries[j];
      if (x.chunk_offset != y.chunk_offset || x.skip_bytes != y.skip_bytes || x.skip_values != y.skip_values || x.skip_bits != y.skip_bits) return false;
    }
  }
  return true;
}
static bool same_batches(const std::vector<SelBatch>& a, const std::vector<SelBatch>& b) {
  if (a.size() != b.size()) return false;
  for (size_t k = 0; k < a.size(); k++)
    if (a[k].start != b[k].start || a[k].len != b[k].len || a[k].pad != b[k].pad) return false;
  return true;
}

// ---- a stripe to plan: types, footer, index, file bytes ---------------------------------------------------------------
struct Stripe {
  RefReader R;
  Projection proj;
  StripeFooter sf;
  std::vector<uint8_t> bytes;
  std::vector<std::vector<uint64_t>> chunk_starts;  // per stream: where its chunks start (compressed)
  uint64_t n_rows = 0;
};
// the positions of one RowIndexEntry field by field: which stream's entry (0 present, 1 data, 2 second) and which member
// (0 chunk_offset, 1 skip_bytes, 2 skip_values, 3 skip_bits); empty: the column records no such entry
static std::vector<std::pair<int, int>> entry_fields(int kind, int enc, bool has_present, bool compressed) {
  for (uint32_t n = 0; n <= 12; n++) {
    std::vector<uint64_t> pos(n + 1, 0);
    EntrySplit sp;
    if (!split_index_entry(kind, enc, has_present, compressed, pos.data(), n, sp)) continue;
    std::vector<std::pair<int, int>> f;
    for (uint32_t j = 0; j < n; j++) {
      std::fill(pos.begin(), pos.end(), 0);
      pos[j] = 1;
      split_index_entry(kind, enc, has_present, compressed, pos.data(), n, sp);
      const orcgpu_stream_entry* es[3] = {&sp.present, &sp.data, &sp.second};
      for (int w = 0; w < 3; w++) {
        if ((w == 0 && !has_present) || (w == 1 && !sp.has_data) || (w == 2 && !sp.has_second)) continue;
        if (es[w]->chunk_offset == 1) f.push_back({w, 0});
        else if (es[w]->skip_bytes == 1) f.push_back({w, 1});
        else if (es[w]->skip_values == 1) f.push_back({w, 2});
        else if (es[w]->skip_bits == 1) f.push_back({w, 3});
      }
    }
    return f;
  }
  return {};
}
static int second_kind_of(int kind, int enc) {
  uint64_t pos[16] = {0};
  EntrySplit sp;
  for (uint32_t n = 0; n <= 12; n++)
    if (split_index_entry(kind, enc, false, false, pos, n, sp)) return sp.has_second ? sp.second_kind : -1;
  return -1;
}

struct Gen {
  std::mt19937_64 rng;
  explicit Gen(uint64_t seed) : rng(seed) {}
  uint64_t upto(uint64_t n) { return n ? rng() % n : 0; }
  bool coin(int one_in = 2) { return upto(one_in) == 0; }

  static constexpr int kFlat[] = {ORCGPU_T_BOOLEAN, ORCGPU_T_BYTE, ORCGPU_T_SHORT, ORCGPU_T_INT, ORCGPU_T_LONG, ORCGPU_T_FLOAT, ORCGPU_T_DOUBLE, ORCGPU_T_STRING,
                                  ORCGPU_T_BINARY, ORCGPU_T_TIMESTAMP, ORCGPU_T_DECIMAL, ORCGPU_T_DATE, ORCGPU_T_VARCHAR, ORCGPU_T_CHAR, ORCGPU_T_TIMESTAMP_INSTANT};
  uint32_t add_type(std::vector<OrcType>& types, int depth, bool odd) {
    const uint32_t id = (uint32_t)types.size();
    types.emplace_back();
    int kind = kFlat[upto(sizeof(kFlat) / sizeof(kFlat[0]))];
    if (depth < 3 && coin(4)) kind = ORCGPU_T_LIST + (int)upto(4);  // LIST, MAP, STRUCT, UNION
    if (odd && coin(40)) kind = 19 + (int)upto(3);                  // a kind the path does not decode
    types[id].kind = kind;
    types[id].precision = (uint32_t)upto(39);
    types[id].scale = (uint32_t)upto(20);
    size_t kids = kind == ORCGPU_T_LIST ? 1 : kind == ORCGPU_T_MAP ? 2 : (kind == ORCGPU_T_STRUCT || kind == ORCGPU_T_UNION) ? upto(4) : 0;
    if (odd && (kind == ORCGPU_T_LIST || kind == ORCGPU_T_MAP) && coin(12)) kids += 1;
    for (size_t k = 0; k < kids; k++) {
      const uint32_t kid = odd && coin(60) ? (uint32_t)(1000 + upto(5)) : add_type(types, depth + 1, odd);
      types[id].subtypes.push_back(kid);
      if (kind == ORCGPU_T_STRUCT && !(odd && coin(10))) types[id].field_names.push_back("f" + std::to_string(k));
    }
    return id;
  }
  void types(FileMetadata& md, bool odd) {
    md.types.clear();
    md.types.emplace_back();
    md.types[0].kind = ORCGPU_T_STRUCT;
    const size_t n = upto(7) + (odd ? 0 : 1);
    for (size_t k = 0; k < n; k++) {
      const uint32_t id = add_type(md.types, 1, odd);
      md.types[0].subtypes.push_back(id);
      if (!(odd && coin(15))) md.types[0].field_names.push_back(odd && coin(10) ? "c0" : "c" + std::to_string(k));
    }
  }
  // the Arrow field a caller would hint for a type -- now and then another one
  SchemaNode hint(const FileMetadata& md, uint32_t id, int depth, int wrong_depth) {
    SchemaNode n;
    n.name = "h" + std::to_string(id);
    if (id >= md.types.size()) return n;
    const OrcType& t = md.types[id];
    static const char* flat[] = {"b", "c", "s", "i", "l", "f", "g", "u", "z", "tsn:", "", "", "", "", "d:20,4", "tdD", "u", "u", "tsu:UTC"};
    if (t.kind >= 0 && t.kind <= 18) n.format = flat[t.kind];
    auto kid = [&](uint32_t k) { return hint(md, k, depth + 1, wrong_depth); };
    if (t.kind == ORCGPU_T_STRUCT || t.kind == ORCGPU_T_UNION) {
      n.format = t.kind == ORCGPU_T_STRUCT ? "+s" : (coin() ? "+us:0,1" : "+ud:0,1");
      for (uint32_t k : t.subtypes) n.kids.push_back(kid(k));
    } else if (t.kind == ORCGPU_T_LIST) {
      n.format = "+l";
      for (uint32_t k : t.subtypes) n.kids.push_back(kid(k));
    } else if (t.kind == ORCGPU_T_MAP) {
      n.format = "+m";
      n.flags = coin() ? 4 : 2;
      SchemaNode e;
      e.format = "+s";
      e.name = "entries";
      for (uint32_t k : t.subtypes) e.kids.push_back(kid(k));
      n.kids.push_back(e);
    }
    if (depth == wrong_depth || coin(25)) {
      static const char* other[] = {"l", "+s", "+l", "+m", "u", "d:10,2,256", "tss:Europe/Berlin", "tsx:", "d:0,1", "+us:0", ""};
      n.format = other[upto(sizeof(other) / sizeof(other[0]))];
      if (coin(3)) n.kids.clear();
    }
    return n;
  }
  void options(RefReader& R, bool odd) {
    const OrcType& root = R.md.types[0];
    const size_t n = root.subtypes.size();
    const int mode = (int)upto(3);
    R.project_all = mode == 0;
    R.by_index = mode == 2;
    for (size_t k = 0; k < n + 1; k++)
      if (coin()) {
        R.projected_roots.push_back((uint32_t)k);
        R.projected_names.push_back("c" + std::to_string(k));
      }
    if (coin(3)) {
      std::vector<SchemaNode> tree;
      const size_t fields = coin(4) ? upto(n + 1) : n;  // (fewer schema fields than columns)
      size_t at = 0;
      for (size_t k = 0; k < n && tree.size() < fields; k++) {
        const std::string nm = k < root.field_names.size() ? root.field_names[k] : std::string();
        const bool take = R.project_all || (R.by_index ? std::find(R.projected_roots.begin(), R.projected_roots.end(), (uint32_t)k) != R.projected_roots.end()
                                                        : std::find(R.projected_names.begin(), R.projected_names.end(), nm) != R.projected_names.end());
        if (!take) continue;
        tree.push_back(hint(R.md, root.subtypes[k], 0, coin(6) ? (int)upto(3) : -1));
        at++;
      }
      set_schema(R, tree);
    }
    if (coin(3)) {
      R.shard_world = 1 + (uint32_t)upto(4);
      R.shard_rank = (uint32_t)upto(R.shard_world);
      R.shard_mode = coin() ? ORCGPU_SHARD_COLUMNS : ORCGPU_SHARD_STRIPES;
    }
    for (size_t k = 0; k < n; k++) {
      const uint32_t id = root.subtypes[k];
      const bool is_string = id < R.md.types.size() && (R.md.types[id].kind == ORCGPU_T_STRING || R.md.types[id].kind == ORCGPU_T_VARCHAR);
      if ((is_string && coin(3)) || (odd && coin(30))) R.dict_names.push_back(k < root.field_names.size() ? root.field_names[k] : std::string());
    }
    R.ts_arrow_target = ORCGPU_ARROW_TIMESTAMP_S + (int)upto(4);
  }

  // a stripe of the projected columns: streams with (compressed) chunked bytes behind them, encodings, and an index whose
  // positions point at chunk starts -- now and then something is off
  void stripe(Stripe& S, bool odd, bool sure = false) {
    RefReader& R = S.R;
    const bool compressed = R.md.compression != ORCGPU_COMP_NONE;
    const uint64_t stride = R.md.row_index_stride;
    const uint64_t n_groups = stride ? (S.n_rows + stride - 1) / stride : 1;
    S.sf = StripeFooter{};
    S.sf.encodings.assign(R.md.types.size(), {ORCGPU_ENC_DIRECT_V2, 0});
    S.bytes.assign(16, 0);
    struct Made { uint32_t column; int kind; };
    std::vector<Made> made;
    for (uint32_t id = 1; id < R.md.types.size(); id++) {
      const OrcType& t = R.md.types[id];
      const bool is_str = t.kind == ORCGPU_T_STRING || t.kind == ORCGPU_T_VARCHAR || t.kind == ORCGPU_T_CHAR;
      if (is_str && coin()) S.sf.encodings[id] = {coin() ? ORCGPU_ENC_DICTIONARY_V2 : ORCGPU_ENC_DICTIONARY, (uint32_t)upto(100)};
      const int enc = S.sf.encodings[id].first;
      if (coin()) made.push_back({id, ORCGPU_S_PRESENT});
      if (coin(5)) made.push_back({id, ORCGPU_S_ROW_INDEX});
      if (t.kind != ORCGPU_T_STRUCT && t.kind != ORCGPU_T_LIST && t.kind != ORCGPU_T_MAP) made.push_back({id, ORCGPU_S_DATA});
      const int second = second_kind_of(t.kind, enc);
      if (second >= 0) made.push_back({id, second});
      if (is_string_dict_column(t.kind, enc)) {
        made.push_back({id, ORCGPU_S_LENGTH});
        made.push_back({id, ORCGPU_S_DICTIONARY_DATA});
      }
    }
    if (odd && coin(8)) made.push_back({(uint32_t)(R.md.types.size() + upto(3)), ORCGPU_S_DATA});
    S.chunk_starts.clear();
    for (auto& m : made) {
      StreamInfo s{m.kind, m.column, 0, S.bytes.size()};
      std::vector<uint64_t> starts;
      const size_t n_chunks = 1 + upto(2 * n_groups + 2);
      const bool big = coin(12);  // (16 KiB or more per row group: whole_stripe_entries takes the stream)
      for (size_t c = 0; c < n_chunks; c++) {
        starts.push_back(S.bytes.size() - s.offset);
        uint64_t len = big ? 16384 * n_groups / n_chunks + upto(64) : upto(300);
        uint64_t h = len << 1;
        if (odd && coin(50)) h = (len + 1 + upto(5000)) << 1;  // (a header that runs past the stream)
        S.bytes.push_back((uint8_t)h), S.bytes.push_back((uint8_t)(h >> 8)), S.bytes.push_back((uint8_t)(h >> 16));
        S.bytes.resize(S.bytes.size() + len, 0x5a);
      }
      if (odd && coin(30)) S.bytes.push_back(1), S.bytes.push_back(2);  // (a tail too short for a header)
      s.length = S.bytes.size() - s.offset;
      S.sf.streams.push_back(s);
      S.chunk_starts.push_back(starts);
    }
    S.sf.index_read = !coin(6);
    if (sure || (S.sf.index_read && !coin(10)))
      for (uint32_t id = 1; id < R.md.types.size(); id++) {
        if (odd && coin(12)) continue;  // (a column without an index)
        const OrcType& t = R.md.types[id];
        const int enc = S.sf.encodings[id].first;
        bool has_present = false;
        for (auto& s : S.sf.streams) has_present = has_present || (s.column == id && s.kind == ORCGPU_S_PRESENT);
        const std::vector<std::pair<int, int>> fields = entry_fields(t.kind, enc, has_present, compressed);
        ColumnIndex ci;
        ci.column = id;
        ci.n_groups = (uint32_t)n_groups + (odd && coin(15) ? 1 : 0);
        ci.per_group = (uint32_t)fields.size() + (odd && coin(15) ? 1 : 0);
        const int second = second_kind_of(t.kind, enc);
        for (uint64_t g = 0; g < ci.n_groups; g++)
          for (uint32_t j = 0; j < ci.per_group; j++) {
            uint64_t v = 0;
            if (j < fields.size()) {
              const int want = fields[j].first == 0 ? ORCGPU_S_PRESENT : fields[j].first == 1 ? ORCGPU_S_DATA : second;
              size_t si = 0;
              while (si < S.sf.streams.size() && !(S.sf.streams[si].column == id && S.sf.streams[si].kind == want)) si++;
              const uint64_t slen = si < S.sf.streams.size() ? S.sf.streams[si].length : 100;
              if (fields[j].second == 0) {
                if (si < S.sf.streams.size() && compressed) v = S.chunk_starts[si][std::min<uint64_t>(S.chunk_starts[si].size() - 1, g * S.chunk_starts[si].size() / ci.n_groups)];
                else v = g * slen / ci.n_groups;
                if (odd && coin(80)) v = upto(slen + 50);  // (beyond the stream, or before the entry in front)
              } else if (fields[j].second == 1) {
                v = compressed ? upto(200) : 0;
                if (odd && coin(80)) v = R.md.block_size + upto(2);
              } else if (fields[j].second == 2) {
                v = coin(10) ? 512 + (odd ? upto(2) : 0) : upto(512);
              } else {
                v = upto(8);
              }
            } else {
              v = upto(9);
            }
            ci.positions.push_back(v);
          }
        ci.has_groups = false;
        S.sf.index.push_back(ci);
      }
  }
};
constexpr int Gen::kFlat[];

// ---- the cases --------------------------------------------------------------------------------------------------------
static RefReader flat_file(const std::vector<int>& kinds) {
  RefReader R;
  R.md.types.emplace_back();
  R.md.types[0].kind = ORCGPU_T_STRUCT;
  for (size_t k = 0; k < kinds.size(); k++) {
    OrcType t;
    t.kind = kinds[k];
    R.md.types[0].subtypes.push_back((uint32_t)R.md.types.size());
    R.md.types[0].field_names.push_back("c" + std::to_string(k));
    R.md.types.push_back(t);
  }
  return R;
}
static SchemaNode field(const char* format, const char* name, std::vector<SchemaNode> kids = {}, int64_t flags = 0) {
  SchemaNode n;
  n.format = format;
  n.name = name;
  n.flags = flags;
  n.kids = std::move(kids);
  return n;
}

static void projection_cases() {
  {
    size_t bad = 0, errors = 0;
    const size_t N = 3000;
    for (size_t i = 0; i < N; i++) {
      Gen G(1000 + i);
      RefReader R;
      const bool odd = i % 3 == 0;
      G.types(R.md, odd);
      G.options(R, odd);
      int rc = 0;
      bad += !same_projection(R, &rc);
      errors += rc != 0;
    }
    if (errors < N / 50 || errors > N / 2) bad++;  // (the generator must reach the error paths, and mostly not)
    report("projection, random", N, bad);
  }
  {
    size_t bad = 0;
    for (int mode = 0; mode < 3; mode++) {
      RefReader R = flat_file({ORCGPU_T_LONG, ORCGPU_T_STRING, ORCGPU_T_DOUBLE, ORCGPU_T_DATE});
      R.project_all = mode == 0;
      R.by_index = mode == 2;
      R.projected_names = {"c3", "c1", "nope"};
      R.projected_roots = {3, 1, 9};
      Projection P;
      bad += !same_projection(R, nullptr, &P);
      bad += P.names != (mode == 0 ? std::vector<std::string>{"c0", "c1", "c2", "c3"} : std::vector<std::string>{"c1", "c3"});
    }
    report("projection, by name, by index, all", 3, bad);
  }
  {
    RefReader R = flat_file({ORCGPU_T_LONG, ORCGPU_T_STRING, ORCGPU_T_DOUBLE});
    set_schema(R, {field("l", "a"), field("u", "b")});
    Projection P;
    size_t bad = !same_projection(R, nullptr, &P);
    bad += P.names != std::vector<std::string>{"a", "b"} || P.cols.size() != 2 || P.cols[1].target != ORCGPU_ARROW_UTF8;
    report("projection, fewer schema fields than columns", 1, bad);
  }
  {
    // c0: struct<f0: struct<f0: long>>; the hint is wrong for the root, then for the field two levels down
    size_t bad = 0;
    for (int wrong = 0; wrong < 2; wrong++) {
      RefReader R = flat_file({ORCGPU_T_STRUCT});
      R.md.types[1].subtypes = {2};
      R.md.types[1].field_names = {"f0"};
      OrcType mid, leaf;
      mid.kind = ORCGPU_T_STRUCT, mid.subtypes = {3}, mid.field_names = {"f0"};
      leaf.kind = ORCGPU_T_LONG;
      R.md.types.push_back(mid);
      R.md.types.push_back(leaf);
      set_schema(R, {field(wrong == 0 ? "+l" : "+s", "r", {field("+s", "m", {field(wrong == 1 ? "tdD" : "l", "x")})})});
      Projection P;
      bad += !same_projection(R, nullptr, &P);
      bad += wrong == 0 ? !(P.cols.size() == 1 && P.cols[0].target == ORCGPU_ARROW_OTHER)
                        : !(P.cols.size() == 3 && P.cols[2].target == ORCGPU_ARROW_DATE32 && P.cols[2].field == "x" && P.cols[2].parent == 2 && P.cols[2].root == 0);
    }
    report("projection, a hint that mismatches at depth 0 and at depth 2", 2, bad);
  }
  {
    size_t bad = 0;
    for (int sorted = 0; sorted < 2; sorted++) {
      RefReader R = flat_file({ORCGPU_T_MAP});
      R.md.types[1].subtypes = {2, 3};
      OrcType k, v;
      k.kind = ORCGPU_T_STRING, v.kind = ORCGPU_T_INT;
      R.md.types.push_back(k);
      R.md.types.push_back(v);
      set_schema(R, {field("+m", "m", {field("+s", "entries", {field("u", "key"), field("i", "value")})}, sorted ? 4 : 2)});
      Projection P;
      bad += !same_projection(R, nullptr, &P);
      bad += !(P.cols.size() == 3 && P.cols[0].target == (sorted ? ORCGPU_ARROW_MAP_SORTED : ORCGPU_ARROW_MAP) && P.cols[1].field == "key" && P.cols[2].target == ORCGPU_ARROW_INT32);
    }
    report("projection, Map with and without the sorted flag", 2, bad);
  }
  {
    RefReader R = flat_file({ORCGPU_T_LONG, ORCGPU_T_LIST});
    R.md.types[2].subtypes = {3, 3};
    OrcType e;
    e.kind = ORCGPU_T_INT;
    R.md.types.push_back(e);
    int rc = 0;
    Projection P;
    size_t bad = !same_projection(R, &rc, &P);
    bad += rc != ORCGPU_OUT_OF_SPEC || P.names.size() != 2 || P.cols.size() != 1;  // (what was walked so far stays)
    report("projection, a List with two subtypes", 1, bad);
  }
  {
    // a Struct that is its own field: followed kMaxTypeDepth deep, then out of spec
    RefReader R = flat_file({ORCGPU_T_STRUCT});
    R.md.types[1].subtypes = {1};
    R.md.types[1].field_names = {"me"};
    int rc = 0;
    Projection P;
    size_t bad = !same_projection(R, &rc, &P);
    bad += rc != ORCGPU_OUT_OF_SPEC || P.cols.size() != (size_t)kMaxTypeDepth + 1;
    report("projection, a type cycle at kMaxTypeDepth", 1, bad);
  }
  {
    size_t bad = 0, calls = 0;
    for (uint32_t world : {2u, 4u}) {
      std::vector<std::string> all;
      for (uint32_t rank = 0; rank < world; rank++, calls++) {
        RefReader R = flat_file({ORCGPU_T_LONG, ORCGPU_T_STRING, ORCGPU_T_BOOLEAN, ORCGPU_T_DECIMAL, ORCGPU_T_INT, ORCGPU_T_STRING, ORCGPU_T_BYTE});
        R.shard_world = world, R.shard_rank = rank, R.shard_mode = ORCGPU_SHARD_COLUMNS;
        set_schema(R, {field("l", "s0"), field("u", "s1"), field("b", "s2"), field("d:20,4", "s3"), field("i", "s4"), field("u", "s5"), field("c", "s6")});
        Projection P;
        bad += !same_projection(R, nullptr, &P);
        all.insert(all.end(), P.names.begin(), P.names.end());
        for (size_t k = 0; k < P.cols.size(); k++) bad += P.names[k] != "s" + std::to_string(P.cols[k].id - 1);  // (the schema's field of the column's position)
      }
      std::sort(all.begin(), all.end());
      bad += all != std::vector<std::string>{"s0", "s1", "s2", "s3", "s4", "s5", "s6"};  // (the ranks' shares partition the columns)
    }
    report("projection, a column shard over 2 and 4 ranks", calls, bad);
  }
  {
    size_t bad = 0;
    for (int columns = 0; columns < 2; columns++) {
      RefReader R = flat_file({ORCGPU_T_LONG, ORCGPU_T_STRING});
      R.project_all = false;
      R.projected_names = {"c0"};
      R.dict_names = {"c1"};
      if (columns) R.shard_world = 2, R.shard_mode = ORCGPU_SHARD_COLUMNS;
      int rc = 0;
      bad += !same_projection(R, &rc);
      bad += rc != (columns ? ORCGPU_OK : ORCGPU_INVALID_ARGUMENT);
      bad += !columns && strcmp(R.err, "dictionary column 'c1' is not among the projected columns");
    }
    report("projection, a dictionary column that is not projected, with and without column sharding", 2, bad);
  }
  {
    // stripe shards: the rule as it stood inline in reader_stage_next and as the lambda of reader_read_metadata_ahead
    size_t bad = 0, calls = 0;
    for (uint32_t world = 1; world <= 5; world++)
      for (uint32_t rank = 0; rank < world; rank++)
        for (int mode : {ORCGPU_SHARD_STRIPES, ORCGPU_SHARD_COLUMNS})
          for (size_t at = 0; at < 12; at++, calls++) {
            ProjectionOptions o;
            o.shard_world = world, o.shard_rank = rank, o.shard_mode = mode;
            const bool other = world > 1 && mode == ORCGPU_SHARD_STRIPES && at % world != rank;
            bad += stripe_is_mine(o, at) != !other;
          }
    report("projection, the stripe shard rule", calls, bad);
  }
}

// one stripe planned by both; `selection` is the reader's, consumed by the call
static bool same_plan(Stripe& S, bool has_predicate, bool pred_ok, const std::vector<uint8_t>& keep, bool has_selection, std::vector<RowSel> selection,
                      StagePlan* plan_out = nullptr) {
  RefReader& R = S.R;
  BytesChunkReader file(S.bytes.data(), S.bytes.size());
  R.reader = &file;
  std::vector<RowSel> sel_ref = selection, sel_new = selection;
  RefPlan ref;
  ref_stage_next(&R, S.sf, S.n_rows, has_predicate, pred_ok, keep, has_selection, sel_ref, ref);
  StripeAsk a;
  a.n_rows = S.n_rows;
  a.stride = R.md.row_index_stride;
  a.batch_size = R.batch_size;
  a.prune = R.prune;
  a.has_filter = R.has_filter;
  a.has_predicate = has_predicate;
  a.predicate_ok = pred_ok;
  a.keep = &keep;
  std::vector<RowSel> share;
  const bool has_share = has_selection && sel_row_count(sel_new) > 0;
  if (has_share) share = sel_split_off(sel_new, S.n_rows);
  int index_reads = 0;
  StagePlan plan = plan_stripe(R.md, S.sf, S.proj, file, a, has_share ? &share : nullptr, [&] { index_reads++; });
  bool same = plan.stages.size() == ref.out.size() && plan.groups_total == ref.groups_total && plan.groups_read == ref.groups_read && index_reads == ref.index_reads &&
              sel_ref.size() == sel_new.size();
  for (size_t k = 0; k < sel_ref.size() && same; k++) same = sel_ref[k].row_count == sel_new[k].row_count && sel_ref[k].skip == sel_new[k].skip;
  uint64_t groups = 0;
  for (size_t k = 0; k < plan.stages.size() && same; k++) {
    const StagePiece& p = plan.stages[k];
    same = same_pieces(p.pieces, ref.out[k].pieces) && p.n_rows == ref.out[k].n_rows && p.has_sel == ref.out[k].has_sel && p.is_piece == ref.out[k].piece &&
           same_batches(p.sel, ref.out[k].sel);
    groups += p.groups;
  }
  same = same && groups == plan.groups_read;
  if (same && !plan.stages.empty()) {  // the column fill of the staging call
    const std::vector<orcgpu_column> c_ref = ref_columns(&R, S.sf), c_new = stripe_columns(R.md, S.sf, S.proj, options_of(R));
    same = c_ref.size() == c_new.size();
    for (size_t k = 0; k < c_ref.size() && same; k++) same = !memcmp(&c_ref[k], &c_new[k], sizeof(orcgpu_column));
  }
  R.reader = nullptr;
  if (plan_out) *plan_out = std::move(plan);
  return same;
}

// a stripe of `kinds` columns, `n_rows` rows, an index that works
static void make_stripe(Stripe& S, const std::vector<int>& kinds, uint64_t n_rows, uint64_t stride, int compression, uint64_t seed) {
  S.R = flat_file(kinds);
  S.R.md.row_index_stride = stride;
  S.R.md.compression = compression;
  S.n_rows = n_rows;
  ref_build(&S.R);
  MetaErr e;
  build_projection(S.R.md, options_of(S.R), S.proj, e);
  Gen G(seed);
  G.stripe(S, false, true);
  S.sf.index_read = true;
}
static std::vector<RowSel> keep_groups(const std::vector<uint8_t>& keep, uint64_t stride) {
  std::vector<RowSel> s;
  for (uint8_t k : keep) s.push_back(RowSel{stride, !k});
  return s;
}

static void plan_cases() {
  {
    size_t bad = 0, pieces = 0, nothing = 0, whole = 0, with_entries = 0;
    const size_t N = 4000;
    for (size_t i = 0; i < N; i++) {
      Gen G(77000 + i);
      Stripe S;
      const bool odd = i % 4 == 0;
      G.types(S.R.md, false);
      G.options(S.R, false);
      S.R.shard_mode = ORCGPU_SHARD_STRIPES;
      static const uint64_t strides[] = {0, 1, 7, 100, 1000, 10000};
      S.R.md.row_index_stride = strides[G.upto(6)];
      S.R.md.compression = G.coin() ? ORCGPU_COMP_NONE : ORCGPU_COMP_ZSTD;
      S.R.md.block_size = 1024 << G.upto(9);
      S.R.batch_size = G.coin(3) ? (uint32_t)std::max<uint64_t>(1, S.R.md.row_index_stride) : (uint32_t)(1 + G.upto(3000));
      S.R.prune = !G.coin(6);
      S.R.has_filter = G.coin(3);
      const uint64_t stride = S.R.md.row_index_stride;
      S.n_rows = 1 + G.upto(stride ? std::min<uint64_t>(40 * stride, 30000) : 5000);
      if (stride && G.coin(4)) S.n_rows = stride * (1 + G.upto(8)) + G.upto(2);
      if (ref_build(&S.R)) continue;
      MetaErr e;
      build_projection(S.R.md, options_of(S.R), S.proj, e);
      G.stripe(S, odd);
      const uint64_t ng = stride ? (S.n_rows + stride - 1) / stride : 0;
      const bool has_predicate = G.coin(), pred_ok = !G.coin(5), has_selection = G.coin();
      std::vector<uint8_t> keep;
      const int dens = 1 + (int)G.upto(6);
      if (!G.coin(10))
        for (uint64_t g = 0; g < ng; g++) keep.push_back(G.upto(dens) == 0);
      std::vector<RowSel> sel;
      for (size_t k = G.upto(8); k > 0; k--) sel.push_back(RowSel{G.upto(2 * S.n_rows / 3 + 2), G.coin()});
      StagePlan plan;
      bad += !same_plan(S, has_predicate, pred_ok, keep, has_selection, sel, &plan);
      nothing += plan.stages.empty();
      for (auto& p : plan.stages) {
        pieces += p.is_piece, whole += !p.is_piece;
        for (auto& s : p.pieces) with_entries += !s.entries.empty();
      }
    }
    if (pieces < N / 20 || nothing < N / 50 || whole < N / 10 || with_entries < 20) bad++;  // (the generator must reach every outcome)
    report("plan, random", N, bad);
  }
  const std::vector<int> kinds = {ORCGPU_T_LONG, ORCGPU_T_DOUBLE, ORCGPU_T_STRING, ORCGPU_T_BOOLEAN};
  {
    Stripe S;
    make_stripe(S, kinds, 5000, 0, ORCGPU_COMP_NONE, 1);
    StagePlan p;
    size_t bad = !same_plan(S, false, false, {}, true, {{100, true}, {50, false}}, &p);
    bad += !(p.stages.size() == 1 && !p.stages[0].is_piece && p.stages[0].has_sel && p.groups_total == 1 && p.groups_read == 1);
    bad += !same_plan(S, true, true, {}, false, {}, &p);  // (a predicate over no row groups: skip_all)
    bad += !p.stages.empty();
    report("plan, stride 0", 2, bad);
  }
  {
    Stripe S;
    make_stripe(S, kinds, 900, 1000, ORCGPU_COMP_ZSTD, 2);
    StagePlan p;
    size_t bad = !same_plan(S, false, false, {}, true, {{100, true}, {50, false}}, &p);
    bad += !(p.stages.size() == 1 && !p.stages[0].is_piece && p.stages[0].sel.size() == 1 && p.stages[0].sel[0].start == 100);
    report("plan, one row group", 1, bad);
  }
  {
    size_t bad = 0;
    for (uint64_t n_rows : {4000u, 4001u}) {
      Stripe S;
      make_stripe(S, kinds, n_rows, 1000, ORCGPU_COMP_ZSTD, 3);
      StagePlan p;
      bad += !same_plan(S, false, false, {}, true, {{n_rows - 1, true}, {1, false}}, &p);
      bad += !(p.groups_total == (n_rows + 999) / 1000 && p.stages.size() == 1 && p.stages[0].is_piece && p.stages[0].n_rows == (n_rows == 4000 ? 1000 : 1) &&
               p.stages[0].sel[0].start == (n_rows == 4000 ? 999 : 0));
    }
    report("plan, n_rows an exact multiple of the stride and one more", 2, bad);
  }
  {
    size_t bad = 0, calls = 0;
    const std::vector<std::vector<uint8_t>> keeps = {{0, 0, 0, 0, 0}, {1, 1, 1, 1, 1}, {1, 0, 0, 0, 0}, {0, 0, 0, 0, 1}, {1, 0, 1, 0, 1}, {0, 1, 0, 1, 0}};
    const size_t want_stages[2][6] = {{0, 1, 1, 1, 3, 2}, {0, 1, 1, 1, 1, 1}};
    for (int filter = 0; filter < 2; filter++)
      for (size_t k = 0; k < keeps.size(); k++, calls++) {
        Stripe S;
        make_stripe(S, kinds, 4500, 1000, ORCGPU_COMP_ZSTD, 4);
        S.R.has_filter = filter;
        StagePlan p;
        bad += !same_plan(S, false, false, {}, true, keep_groups(keeps[k], 1000), &p);
        bad += p.stages.size() != want_stages[filter][k];
        if (k == 1) bad += p.stages[0].is_piece || p.groups_read != 5;              // (the full range: not usable, the stripe whole)
        // (a row filter: one run, first to last -- which for groups 0, 2 and 4 is the full range again: the stripe whole)
        if (k == 4) bad += p.groups_read != (filter ? 5u : 3u) || p.stages[0].is_piece != !filter;
        if (k == 4 && filter) bad += !(p.stages[0].sel.size() == 3 && p.stages[0].sel[1].start == 2000 && p.stages[0].sel[2].len == 500);
        if (k == 5) bad += p.groups_read != (filter ? 3u : 2u) || !p.stages[0].is_piece || p.stages[0].n_rows != (filter ? 3000u : 1000u);
        if (k == 5 && filter) bad += !(p.stages[0].sel.size() == 2 && p.stages[0].sel[0].start == 0 && p.stages[0].sel[1].start == 2000);
      }
    report("plan, a selection that keeps nothing, everything, the first, the last, every other group; with and without a row filter", calls, bad);
  }
  {
    Stripe S;
    make_stripe(S, kinds, 6000, 1000, ORCGPU_COMP_NONE, 5);
    StagePlan p;
    size_t bad = !same_plan(S, true, true, {1, 1, 0, 1, 1, 1}, false, {}, &p);
    bad += !(p.stages.size() == 2 && p.stages[0].n_rows == 2000 && p.stages[1].n_rows == 3000 && p.groups_read == 5 && p.stages[1].sel[0].start == 0);
    report("plan, predicate keep-lists that merge neighbours", 1, bad);
  }
  {
    Stripe S;
    make_stripe(S, kinds, 6000, 1000, ORCGPU_COMP_NONE, 6);
    S.R.batch_size = 1024;
    StagePlan p;
    size_t bad = !same_plan(S, true, false, {0, 0, 0, 0, 0, 0}, false, {}, &p);
    bad += !(p.stages.size() == 1 && !p.stages[0].is_piece && !p.stages[0].has_sel && p.stages[0].sel.empty());  // (every row in the batches it has anyway: none)
    report("plan, a predicate that fails and therefore selects all", 1, bad);
  }
  {
    Stripe S;
    make_stripe(S, kinds, 6000, 1000, ORCGPU_COMP_ZSTD, 7);
    StagePlan p;
    size_t bad = !same_plan(S, true, true, {0, 1, 1, 0, 1, 0}, true, {{1500, true}, {3000, false}, {1500, true}}, &p);
    bad += !(p.stages.size() == 2 && p.stages[0].n_rows == 2000 && p.stages[0].sel[0].start == 500 && p.stages[1].n_rows == 1000 && p.stages[1].sel[0].len == 500);
    report("plan, predicate and selection intersected", 1, bad);
  }
  {
    // stripes of 3000 rows dealt to two ranks: rank 1 passes stripe 0 on and plans stripe 1 with what is left
    Stripe S;
    make_stripe(S, kinds, 3000, 1000, ORCGPU_COMP_ZSTD, 8);
    const orcgpu_row_selector given[] = {{2000, 1}, {500, 1}, {0, 0}, {1000, 0}, {10000, 1}};  // (orcgpu_reader_set_row_selection)
    std::vector<RowSel> sel = sel_normalise(given, 5);
    ProjectionOptions o;
    o.shard_world = 2, o.shard_rank = 1;
    size_t bad = stripe_is_mine(o, 0) || !stripe_is_mine(o, 1);
    (void)sel_split_off(sel, 3000);
    StagePlan p;
    bad += !same_plan(S, false, false, {}, true, sel, &p);
    bad += !(p.stages.size() == 1 && p.stages[0].is_piece && p.stages[0].n_rows == 1000 && p.stages[0].sel[0].start == 0 && p.stages[0].sel[0].len == 500);
    report("plan, another rank's stripe consuming its share of the selection", 1, bad);
  }
  {
    Stripe S;
    make_stripe(S, kinds, 5000, 1000, ORCGPU_COMP_ZSTD, 9);
    S.R.batch_size = 600;
    StagePlan p;
    size_t bad = !same_plan(S, false, false, {}, true, {{1700, true}, {600, false}, {1700, true}, {10, false}}, &p);
    bad += !(p.stages.size() == 2 && p.stages[0].n_rows == 2000 && p.stages[0].sel.size() == 1 && p.stages[0].sel[0].start == 700 && p.stages[0].sel[0].len == 600 &&
             p.stages[1].n_rows == 1000 && p.stages[1].sel[0].start == 0);
    report("plan, a batch that straddles a group boundary", 1, bad);
  }
  {
    size_t bad = 0;
    for (uint32_t batch : {1000u, 999u, 7u}) {
      Stripe S;
      make_stripe(S, kinds, 5000, 1000, ORCGPU_COMP_NONE, 10);
      S.R.batch_size = batch;
      bad += !same_plan(S, true, true, {1, 1, 1, 1, 1}, false, {});
      bad += !same_plan(S, true, true, {0, 1, 0, 1, 1}, true, {{4990, false}});
    }
    report("plan, batch_size equal to the stride and coprime with it", 6, bad);
  }
}

// one column, one DATA stream (and PRESENT), positions given by hand
struct OneStream {
  Stripe S;
  void make(int kind, bool compressed, bool present, const std::vector<std::vector<uint64_t>>& entries, uint64_t data_len, int enc = ORCGPU_ENC_DIRECT_V2) {
    S.R = flat_file({kind});
    S.R.md.compression = compressed ? ORCGPU_COMP_ZSTD : ORCGPU_COMP_NONE;
    S.R.md.row_index_stride = 1000;
    S.R.md.block_size = 65536;
    S.n_rows = 1000 * entries.size();
    ref_build(&S.R);
    MetaErr e;
    build_projection(S.R.md, options_of(S.R), S.proj, e);
    S.sf = StripeFooter{};
    S.sf.encodings = {{0, 0}, {enc, 10}};
    S.sf.index_read = true;
    S.bytes.assign(data_len + 64, 0);
    if (present) S.sf.streams.push_back(StreamInfo{ORCGPU_S_PRESENT, 1, 32, 0});
    S.sf.streams.push_back(StreamInfo{ORCGPU_S_DATA, 1, data_len, 32});
    ColumnIndex ci;
    ci.column = 1;
    ci.n_groups = (uint32_t)entries.size();
    ci.per_group = (uint32_t)entries[0].size();
    for (auto& en : entries) ci.positions.insert(ci.positions.end(), en.begin(), en.end());
    S.sf.index.push_back(ci);
  }
  void chunk_header(uint64_t at, uint64_t len) {
    S.bytes[32 + at] = (uint8_t)(len << 1), S.bytes[33 + at] = (uint8_t)(len >> 7), S.bytes[34 + at] = (uint8_t)(len >> 15);
  }
  // groups [g0, g1) by both; `usable`, and the DATA piece when they are
  bool same(uint64_t g0, uint64_t g1, bool* usable, StreamPiece* data = nullptr) {
    BytesChunkReader file(S.bytes.data(), S.bytes.size());
    S.R.reader = &file;
    std::vector<StreamPiece> a, b;
    const uint64_t ng = S.sf.index[0].n_groups;
    const bool ua = ref_row_group_pieces(&S.R, S.sf, ng, g0, g1, a), ub = row_group_pieces(S.R.md, S.sf, S.proj, file, ng, g0, g1, b);
    S.R.reader = nullptr;
    *usable = ub;
    if (data && ub) *data = b.back();
    return ua == ub && same_pieces(a, b);
  }
};

static void piece_cases() {
  bool ok = false;
  StreamPiece pc;
  {
    size_t bad = 0;
    OneStream T;
    T.make(ORCGPU_T_LONG, false, false, {{0, 0}, {4000, 17}, {9000, 3}}, 20000);
    bad += !T.same(1, 2, &ok, &pc) || !ok || !(pc.start == 4000 && pc.end == 9000 + 8192 && pc.skip_values == 17 && pc.skip_bytes == 0);
    bad += !T.same(1, 3, &ok, &pc) || !ok || pc.end != 20000;
    // (an uncompressed DOUBLE stream records bytes only; a non-zero skip_bytes can only come with compressed positions read as
    // uncompressed ones: the column then records another count of positions and the entry does not split)
    T.make(ORCGPU_T_DOUBLE, false, false, {{0, 0}, {4000, 5}, {9000, 0}}, 20000);
    bad += !T.same(1, 2, &ok) || ok;
    report("pieces, uncompressed, with and without a non-zero skip_bytes", 3, bad);
  }
  {
    size_t bad = 0;
    OneStream T;
    T.make(ORCGPU_T_LONG, true, false, {{0, 0, 0}, {100, 50, 7}, {300, 10, 0}}, 1000);
    T.chunk_header(300, 200);
    T.chunk_header(503, 100);
    bad += !T.same(1, 2, &ok, &pc) || !ok || !(pc.start == 100 && pc.end == 300 + 203 + 103 && pc.skip_bytes == 50 && pc.skip_values == 7);
    T.make(ORCGPU_T_LONG, true, false, {{0, 0, 0}, {100, 50, 7}, {300, 10, 0}}, 505);  // (the second header missing: two bytes left)
    T.chunk_header(300, 200);
    bad += !T.same(1, 2, &ok) || ok;
    T.make(ORCGPU_T_LONG, true, false, {{0, 0, 0}, {100, 50, 7}, {300, 10, 0}}, 1000);
    T.chunk_header(300, 698);  // (a header length running past the stream by one byte)
    bad += !T.same(1, 2, &ok) || ok;
    T.chunk_header(300, 697);  // (... and one that ends with it: no second chunk)
    bad += !T.same(1, 2, &ok, &pc) || !ok || pc.end != 1000;
    T.make(ORCGPU_T_LONG, true, false, {{0, 0, 0}, {100, 50, 7}, {1001, 10, 0}}, 1000);  // (an entry beyond s.length)
    bad += !T.same(1, 2, &ok) || ok;
    report("pieces, compressed: the second header missing, a header length past the stream, an entry beyond the stream", 5, bad);
  }
  {
    size_t bad = 0;
    for (uint64_t v : {512u, 513u}) {
      OneStream T;
      T.make(ORCGPU_T_LONG, false, false, {{0, 0}, {4000, v}, {9000, 3}}, 20000);
      bad += !T.same(1, 2, &ok) || ok != (v == 512);
    }
    report("pieces, skip_values 512 and 513", 2, bad);
  }
  {
    size_t bad = 0;
    for (uint64_t v : {7u, 8u}) {
      OneStream T;  // (a Boolean column: offset, values of the byte run, bits)
      T.make(ORCGPU_T_BOOLEAN, false, false, {{0, 0, 0}, {40, 3, v}, {90, 0, 0}}, 200);
      bad += !T.same(1, 2, &ok, &pc) || ok != (v == 7) || (ok && pc.skip_bits != 7);
    }
    report("pieces, skip_bits 7 and 8", 2, bad);
  }
  {
    OneStream T;
    T.make(ORCGPU_T_LONG, false, false, {{0, 0}, {4000, 17}, {9000, 3}}, 20000);
    T.S.sf.index[0].n_groups = 4;
    T.S.sf.index[0].positions.resize(8, 0);
    BytesChunkReader file(T.S.bytes.data(), T.S.bytes.size());
    T.S.R.reader = &file;
    std::vector<StreamPiece> a, b;
    size_t bad = ref_row_group_pieces(&T.S.R, T.S.sf, 3, 1, 2, a) || row_group_pieces(T.S.R.md, T.S.sf, T.S.proj, file, 3, 1, 2, b);
    report("pieces, an index with the wrong n_groups", 1, bad);
  }
  {
    OneStream T;
    T.make(ORCGPU_T_STRING, false, true, {{0, 0, 0, 0, 0}, {4, 1, 2, 4000, 17}, {9, 0, 0, 9000, 3}}, 20000, ORCGPU_ENC_DICTIONARY_V2);
    T.S.sf.streams.push_back(StreamInfo{ORCGPU_S_LENGTH, 1, 10, 8});
    T.S.sf.streams.push_back(StreamInfo{ORCGPU_S_DICTIONARY_DATA, 1, 12, 16});
    BytesChunkReader file(T.S.bytes.data(), T.S.bytes.size());
    T.S.R.reader = &file;
    std::vector<StreamPiece> a, b;
    size_t bad = !ref_row_group_pieces(&T.S.R, T.S.sf, 3, 1, 2, a) || !row_group_pieces(T.S.R.md, T.S.sf, T.S.proj, file, 3, 1, 2, b) || !same_pieces(a, b);
    bad += !(b.size() == 4 && b[0].start == 4 && b[0].skip_values == 1 && b[0].skip_bits == 2 && b[1].start == 4000 && b[2].start == 0 && b[2].end == 10 &&
             b[3].start == 0 && b[3].end == 12);  // (the dictionary's LENGTH and DICTIONARY_DATA: whole)
    report("pieces, a dictionary column's LENGTH and DICTIONARY_DATA streams", 1, bad);
  }
  {
    OneStream T;
    T.make(ORCGPU_T_LONG, false, false, {{0, 0}, {4000, 17}, {3999, 3}}, 20000);
    size_t bad = !T.same(1, 2, &ok) || ok;
    report("pieces, e1.chunk_offset < e0.chunk_offset", 1, bad);
  }
  {
    size_t bad = 0;
    for (uint64_t len : {3u * 16384 - 1, 3u * 16384}) {
      OneStream T;
      T.make(ORCGPU_T_LONG, false, false, {{0, 0}, {4000, 17}, {9000, 3}}, len);
      std::vector<StreamPiece> a = whole_stripe_pieces(T.S.sf, T.S.proj), b = a;
      ref_whole_stripe_entries(&T.S.R, T.S.sf, 3, a);
      whole_stripe_entries(T.S.R.md, T.S.sf, 3, b);
      bad += !same_pieces(a, b) || b[0].entries.size() != (len == 3u * 16384 ? 2u : 0u);
    }
    report("entries, a stream just under and exactly at 16384 bytes per group", 2, bad);
  }
  {
    OneStream T;
    T.make(ORCGPU_T_LONG, true, false, {{0, 0, 0}, {4000, 17, 1}, {9000, 65537, 3}, {9500, 0, 0}}, 4 * 16384);  // (skip_bytes beyond the block size)
    std::vector<StreamPiece> a = whole_stripe_pieces(T.S.sf, T.S.proj), b = a;
    ref_whole_stripe_entries(&T.S.R, T.S.sf, 4, a);
    whole_stripe_entries(T.S.R.md, T.S.sf, 4, b);
    size_t bad = !same_pieces(a, b) || !b[0].entries.empty();
    report("entries, a bad entry that clears the list", 1, bad);
  }
}

static void grouping_cases() {
  const uint64_t MB = 1u << 20;
  const std::vector<size_t> sizes = {0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 33};
  const std::vector<uint64_t> bytes = {0, 1, 8 * MB - 1, 8 * MB, 48 * MB - 1, 48 * MB, 64 * MB - 1, 64 * MB, 64 * MB + 1, 200 * MB};
  size_t bad = 0, calls = 0;
  for (size_t q : sizes)
    for (uint64_t b : bytes) {
      bad += stager_has_room(q, b, 0) != ref_serial_more(q, b);
      for (uint32_t prefetch : {1u, 2u, 4u, 8u}) bad += stager_has_room(q, b, prefetch) != ref_stager_room(q, b, prefetch);
      calls += 5;
    }
  report("grouping, the stager has room: queue sizes and byte totals at each constant and one below; prefetch 1, 2, 4", calls, bad);
  bad = calls = 0;
  for (size_t q : sizes)
    for (uint64_t b : bytes)
      for (bool pieces_only : {false, true}) bad += decoder_should_wake(q, b, pieces_only) != ref_decoder_wake(q, b, pieces_only), calls++;
  bad += decoder_should_wake(1, 8 * MB, true) || !decoder_should_wake(1, 8 * MB, false) || !decoder_should_wake(1, 48 * MB, true) || !decoder_should_wake(32, 0, true);
  report("grouping, the decoder should wake: pieces only against mixed", calls, bad);
  bad = calls = 0;
  for (size_t g : sizes)
    for (uint64_t b : bytes)
      for (uint64_t next : {uint64_t(0), uint64_t(1), 8 * MB, 64 * MB})
        for (size_t room : {0u, 1u, 2u, 4u, 8u}) bad += joins_group(g, b, next, room) != ref_joins(g, b, next, room), calls++;
  bad += kGroupMaxPieces != 32 || kGroupMaxBytes != 64 * MB || kWakeBytesPieces != 48 * MB || kWakeBytesMixed != 8 * MB || kEntriesMinBytesPerGroup != 16384;
  report("grouping, the next staged piece joins this group", calls, bad);
}

int main() {
  projection_cases();
  plan_cases();
  piece_cases();
  grouping_cases();
  printf("checked %d cases, %d mismatches\n", g_cases, g_mismatches);
  return g_mismatches ? 1 : 0;
}
