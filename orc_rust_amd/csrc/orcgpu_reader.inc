// orcgpu_reader.inc -- host-side mirror of the reference's reader API for this path (C++ above the
// C ABI, because the reference is compiled code and there is no Rust toolchain in the image):
//
//   ChunkReader                      src/reader/mod.rs:27-76      (len / get_bytes; File and Bytes)
//   read_metadata                    src/reader/metadata.rs:180-247 (PostScript, Footer; hand-written
//                                    protobuf wire reader: format/orc_proto.proto, SURVEY Appendix C)
//   Stripe::new / StreamMap          src/stripe.rs:127-182, :311-336
//   ProjectionMask::{all,named_roots} src/projection.rs:30-69
//   ArrowReaderBuilder               src/arrow_reader.rs:39-231   (try_new, with_batch_size,
//                                    with_projection, with_file_byte_range, with_timestamp_precision, build)
//   ArrowReader / Cursor             src/arrow_reader.rs:233-392  (next, total_row_count)
//
// Compressed file tails and stripe footers are expanded with the SAME GPU block decompressors as
// the data streams (there is no CPU codec in the product).  Only flat root columns are decoded;
// projecting a nested column is UnsupportedTypeVariant (SURVEY 2 #16: out of scope).
#include <cstdio>
#include <memory>

#include "orcgpu_meta.inc"
#include "orcgpu_dictionary_names.inc"
namespace orcgpu_host {

struct SectionCopy {
  const uint8_t* src;
  uint8_t* dst;
  uint64_t n;
};
__global__ void sections_pack_kernel(const SectionCopy* jobs) {
  const SectionCopy j = jobs[blockIdx.x];
  for (uint64_t i = threadIdx.x; i < j.n; i += blockDim.x) j.dst[i] = j.src[i];
}

// Expand ORC-framed metadata sections on the GPU (Decompressor::read_to_end, metadata.rs:323-337): the same path the stripe
// streams take -- host framing scan, block decoders, finalize (one contiguous plain stream each) --, all sections in one go.
int decompress_sections(orcgpu_ctx* ctx, const std::vector<std::vector<uint8_t>>& raws, int compression, uint64_t block_size,
                        std::vector<std::vector<uint8_t>>& outs) {
  const size_t n = raws.size();
  outs.assign(n, {});
  if (compression == ORCGPU_COMP_NONE) {
    for (size_t k = 0; k < n; k++) outs[k] = raws[k];
    return ORCGPU_OK;
  }
  if (!block_size) block_size = 262144;
  std::vector<StagedStream> ss(n);
  Plan P;
  std::vector<uint64_t> o_dst(n, 0);
  uint64_t src_total = 0;
  bool any = false;
  for (size_t k = 0; k < n; k++) {
    ss[k].column_id = (uint32_t)k;
    ss[k].kind = 0;
    ss[k].off = src_total;
    ss[k].len = raws[k].size();
    src_total += align_up(raws[k].size() + ORC_PAD);
    scan_chunks(raws[k].data(), raws[k].size(), compression, block_size, ss[k]);
    if (ss[k].framing_error) return ORCGPU_IO_ERROR;
    any = any || !ss[k].chunks.empty();
  }
  if (!any) return ORCGPU_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  orcgpu_staged tmp;
  tmp.ctx = ctx;
  tmp.desc.compression = compression;
  tmp.desc.block_size = block_size;
  const uint64_t o_src = P.scratch.take(src_total + ORC_PAD), o_scal = P.scratch.take(16 * n + 64);
  for (size_t k = 0; k < n; k++) {
    uint64_t cap_total = 0;
    for (auto& c : ss[k].chunks) cap_total += c.plain_cap;
    o_dst[k] = P.scratch.take(cap_total + ORC_PAD);
    if (!ss[k].chunks.empty()) P.decomp.push_back(DecompStream{&tmp, &ss[k], o_dst[k], (uint32_t)(2 * k), (uint32_t)(2 * k + 1)});
  }
  const uint64_t pack_cap = P.scratch.off - o_dst[0];
  const uint64_t o_pack = P.scratch.take(pack_cap + 64), o_jobs = P.scratch.take(n * sizeof(SectionCopy) + 64);
  DecompPlan DP;
  int rc = plan_decompress(P, DP);
  if (rc) return rc;
  (void)hipStreamSynchronize(ctx->stream);
  ctx->upload_reset();
  if (!ctx->scratch.ensure(P.scratch.off + kAlign) || !ctx->ensure_pinned(DP.table_bytes + 64)) {
    set_err(ctx, "out of memory while expanding a metadata section");
    return ORCGPU_HIP_ERROR;
  }
  uint8_t* S = ctx->scratch.p;
  tmp.dev = S + o_src;
  uint64_t* d_scal = reinterpret_cast<uint64_t*>(S + o_scal);
  HIP_TRY(ctx, hipMemsetAsync(d_scal, 0, 16 * n + 64, ctx->stream));
  {
    // (one copy up for all sections, one copy back for all of them: a copy of its own for each would cost more than the kernels)
    std::vector<uint8_t> up(src_total, 0);
    for (size_t k = 0; k < n; k++)
      if (!raws[k].empty()) memcpy(up.data() + ss[k].off, raws[k].data(), raws[k].size());
    HIP_TRY(ctx, ctx->upload(S + o_src, up.data(), up.size(), ctx->stream));
  }
  rc = launch_decompress(ctx, P, DP, S, d_scal, ctx->pinned);
  tmp.dev = nullptr;  // (borrowed: part of the workspace)
  if (rc) return rc;
  std::vector<uint64_t> h_scal(2 * n + 2, 0);
  HIP_TRY(ctx, hipMemcpyAsync(h_scal.data(), d_scal, 16 * n, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t k = 0; k < n; k++)
    if (h_scal[2 * k + 1]) {
      set_err(ctx, "a metadata chunk failed to decompress");
      return ORCGPU_BUILD_DECODER;
    }
  // (the sections lie in the workspace a block size or more apart, whatever they hold: packed by a kernel, one copy back)
  std::vector<SectionCopy> jobs(n);
  uint64_t total = 0;
  for (size_t k = 0; k < n; k++) {
    jobs[k] = SectionCopy{S + o_dst[k], S + o_pack + total, h_scal[2 * k]};
    total += h_scal[2 * k];
  }
  if (total > pack_cap) return ORCGPU_UNEXPECTED;
  std::vector<uint8_t> back(total);
  if (total) {
    HIP_TRY(ctx, ctx->upload(S + o_jobs, jobs.data(), n * sizeof(SectionCopy), ctx->stream));
    hipLaunchKernelGGL(sections_pack_kernel, dim3((uint32_t)n), dim3(256), 0, ctx->stream, reinterpret_cast<const SectionCopy*>(S + o_jobs));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(back.data(), S + o_pack, total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  for (size_t k = 0; k < n; k++) outs[k].assign(back.data() + (jobs[k].dst - (S + o_pack)), back.data() + (jobs[k].dst - (S + o_pack)) + jobs[k].n);
  return ORCGPU_OK;
}
int decompress_section(orcgpu_ctx* ctx, const std::vector<uint8_t>& raw, int compression, uint64_t block_size, std::vector<uint8_t>& out) {
  std::vector<std::vector<uint8_t>> raws(1, raw), outs;
  int rc = decompress_sections(ctx, raws, compression, block_size, outs);
  if (!rc) out = std::move(outs[0]);
  return rc;
}

int read_metadata(orcgpu_ctx* ctx, ChunkReader& r, FileMetadata& md) {
  const uint64_t file_len = r.len();
  if (file_len == 0) {
    set_err(ctx, "empty file");
    return ORCGPU_OUT_OF_SPEC;
  }
  const uint64_t tail_len = std::min<uint64_t>(file_len, 16 * 1024);  // DEFAULT_FOOTER_SIZE (metadata.rs:60)
  std::vector<uint8_t> tail;
  if (!r.get_bytes(file_len - tail_len, tail_len, tail)) return ORCGPU_IO_ERROR;
  MetaErr e;
  uint64_t ps_len = 0, footer_length = 0;
  int rc = parse_postscript(tail.data(), tail.size(), md, ps_len, footer_length, e);
  if (rc) {
    if (e.msg[0]) set_err(ctx, "%s", e.msg);
    return rc;
  }
  const uint64_t footer_end = file_len - 1 - ps_len;
  if (footer_length > footer_end) return ORCGPU_OUT_OF_SPEC;
  std::vector<uint8_t> raw_footer;
  if (!r.get_bytes(footer_end - footer_length, footer_length, raw_footer)) return ORCGPU_IO_ERROR;
  std::vector<uint8_t> footer;
  rc = decompress_section(ctx, raw_footer, md.compression, md.block_size, footer);
  if (rc) return rc;
  rc = parse_footer(footer.data(), footer.size(), md, e);
  if (rc && e.msg[0]) set_err(ctx, "%s", e.msg);
  return rc;
}

int stripe_footer_raw(orcgpu_ctx* ctx, ChunkReader& r, const StripeInfo& si, std::vector<uint8_t>& raw) {
  MetaErr e;
  const int rc = stripe_footer_raw(r, si, raw, e);
  if (rc && e.msg[0]) set_err(ctx, "%s", e.msg);
  return rc;
}

int parse_stripe_footer(orcgpu_ctx* ctx, const StripeInfo& si, const std::vector<uint8_t>& plain, StripeFooter& sf) {
  MetaErr e;
  const int rc = parse_stripe_footer(si, plain, sf, e);
  if (rc && e.msg[0]) set_err(ctx, "%s", e.msg);
  return rc;
}

int read_stripe_footer(orcgpu_ctx* ctx, ChunkReader& r, const FileMetadata& md, const StripeInfo& si, StripeFooter& sf) {
  std::vector<uint8_t> raw, plain;
  int rc = stripe_footer_raw(ctx, r, si, raw);
  if (!rc) rc = decompress_section(ctx, raw, md.compression, md.block_size, plain);
  return rc ? rc : parse_stripe_footer(ctx, si, plain, sf);
}

// The footers of several stripes, their sections expanded by ONE call of the GPU decompressors (a call costs a launch chain and
// two host round trips however little it expands).  out[k] <- stripe infos[k]; the count of footers read is returned, and when
// that is short of infos.size(), *rc_out says why footer number `count` could not be read (ctx->err holds the message).
size_t read_stripe_footers(orcgpu_ctx* ctx, ChunkReader& r, const FileMetadata& md, const std::vector<const StripeInfo*>& infos,
                           std::vector<StripeFooter>& out, int* rc_out) {
  const size_t n = infos.size();
  out.assign(n, StripeFooter{});
  *rc_out = 0;
  std::vector<std::vector<uint8_t>> raws(n), plains;
  bool batched = n > 1;
  for (size_t k = 0; k < n && batched; k++) batched = stripe_footer_raw(ctx, r, *infos[k], raws[k]) == ORCGPU_OK;
  if (batched) batched = decompress_sections(ctx, raws, md.compression, md.block_size, plains) == ORCGPU_OK;
  for (size_t k = 0; k < n; k++) {
    // (anything wrong in the batch: one at a time, so that the stripes in front of the bad one are still read)
    int rc = batched ? parse_stripe_footer(ctx, *infos[k], plains[k], out[k]) : read_stripe_footer(ctx, r, md, *infos[k], out[k]);
    if (rc) {
      *rc_out = rc;
      return k;
    }
  }
  return n;
}

// Stripe::read_row_indexes (stripe.rs:266-309, row_index.rs:204-226): the ROW_INDEX streams of `columns`, expanded by the GPU
// decompressors in one go, parsed into position lists.  Columns without such a stream get no entry.
// want_stats: also the row groups' statistics and the columns' BLOOM_FILTER (else BLOOM_FILTER_UTF8) streams (row_index.rs:228-330)
int read_stripe_index(orcgpu_ctx* ctx, ChunkReader& r, const FileMetadata& md, StripeFooter& sf, const std::vector<uint32_t>& columns, bool want_stats) {
  sf.index.clear();
  sf.index_read = true;
  std::vector<std::vector<uint8_t>> raws, plains;
  IndexSections is;
  int rc = index_gather(r, sf, columns, want_stats, raws, is);
  if (rc || raws.empty()) return rc;
  rc = decompress_sections(ctx, raws, md.compression, md.block_size, plains);
  return rc ? rc : index_parse(sf, is, plains, want_stats);
}

// The indexes of several stripes by ONE call of the GPU decompressors.  A stripe whose index cannot be read or parsed is left
// with none (index_read set): it is decoded whole.
void read_stripe_indexes(orcgpu_ctx* ctx, ChunkReader& r, const FileMetadata& md, const std::vector<StripeFooter*>& sfs,
                         const std::vector<uint32_t>& columns, bool want_stats) {
  std::vector<std::vector<uint8_t>> raws, plains;
  std::vector<IndexSections> is(sfs.size());
  bool batched = sfs.size() > 1;
  for (size_t k = 0; k < sfs.size() && batched; k++) batched = index_gather(r, *sfs[k], columns, want_stats, raws, is[k]) == ORCGPU_OK;
  if (batched && !raws.empty()) batched = decompress_sections(ctx, raws, md.compression, md.block_size, plains) == ORCGPU_OK;
  for (size_t k = 0; k < sfs.size(); k++) {
    StripeFooter& sf = *sfs[k];
    int rc;
    if (batched) {
      sf.index.clear();
      sf.index_read = true;
      rc = is[k].n ? index_parse(sf, is[k], plains, want_stats) : ORCGPU_OK;
    } else {
      rc = read_stripe_index(ctx, r, md, sf, columns, want_stats);  // (anything wrong in the batch: one stripe at a time)
    }
    if (rc) {
      sf.index.clear();
      sf.index_read = true;
    }
  }
}

}  // namespace orcgpu_host

// ---- ArrowReaderBuilder + ArrowReader behind one handle -----------------------------------------------------
struct orcgpu_reader {
  orcgpu_ctx* ctx = nullptr;
  std::unique_ptr<orcgpu_host::ChunkReader> reader;
  orcgpu_host::FileMetadata md;
  uint32_t batch_size = 8192;                 // DEFAULT_BATCH_SIZE (arrow_reader.rs:37)
  bool project_all = true;
  std::vector<std::string> projected_names;   // ProjectionMask::named_roots
  bool has_range = false;
  uint64_t range_start = 0, range_end = 0;    // with_file_byte_range
  int ts_arrow_target = ORCGPU_ARROW_TIMESTAMP_NS;
  // iteration state (ArrowReader)
  bool built = false;
  std::vector<size_t> stripe_order;           // Cursor::get_stripe_metadatas
  size_t next_stripe = 0;
  orcgpu_result* current = nullptr;
  uint32_t next_batch = 0;
  std::vector<std::string> col_names;         // of the projected ROOT columns
  std::vector<uint32_t> col_ids;              // every projected column: roots, and below a Struct its fields (pre-order)
  std::vector<uint32_t> col_parent;           // ... 1 + index in col_ids of the Struct a column is a field of (0: a root)
  std::vector<std::string> col_field;         // ... its field name there
  bool by_index = false;                      // ProjectionMask::roots
  std::vector<uint32_t> projected_roots;
  bool has_schema = false;                    // with_schema: per projected column, in order
  std::vector<int> schema_target;
  std::vector<uint32_t> schema_precision, schema_scale;
  std::vector<std::string> schema_names;
  // ... the hinted fields as a tree (nested columns take nested hints: array_decoder/mod.rs:464-505), and per projected column
  // (col_ids order, nested columns included) what the tree says about it
  struct SchemaNode {
    std::string format, name;
    int64_t flags = 0;
    std::vector<SchemaNode> kids;
  };
  std::vector<SchemaNode> schema_tree;
  uint32_t shard_rank = 0, shard_world = 1;   // orcgpu_reader_set_shard
  int shard_mode = ORCGPU_SHARD_STRIPES;
  std::vector<int> col_target;
  std::vector<uint32_t> col_precision, col_scale;
  std::vector<std::string> dict_names;        // orcgpu_reader_set_dictionary_columns: root columns (file names) read as Dictionary(Int32, Utf8)
  std::vector<uint8_t> col_dict;              // ... per projected column (col_ids order)
  bool has_selection = false;                 // with_row_selection
  std::vector<RowSel> selection;              // what is left of it for the stripes to come
  // ---- read-ahead (the analogue of async_arrow_reader.rs:165-280, whose state machine fetches the next stripe while the
  // caller consumes the batches of the current one).  Two threads of the reader own its GPU calls: the STAGER reads the
  // streams of the stripes to come from the file and stages them in HBM (copy stream); the DECODER takes the stripes staged
  // so far -- several per call when it is the slower of the two: short stripes then share their kernel launches --, decodes
  // them, starts their copies back to the host (device-to-host stream) and queues them.  The caller's thread only waits for
  // a copy and hands out views of the pinned host buffers.  In steady state reading + staging (k + 1), decoding (k) and the
  // copy back of (k - 1) overlap.  prefetch = 0: everything in the caller's thread, one stripe after the other. ----
  uint32_t prefetch = 2;                      // decoded stripes the reader may be ahead of the caller
  struct Ready {
    orcgpu_result* res = nullptr;
    int rc = 0;
    std::string err;
  };
  std::vector<orcgpu_host::StripeFooter> footers;  // of the stripes of stripe_order, read (through the GPU decompressors) before the threads start
  bool footers_read = false;                  // ... and then: why the reading stopped early, if it did
  int footers_rc = 0;
  std::string footers_err;
  std::thread stager, decoder;
  std::mutex m;
  std::condition_variable cv_room, cv_ready, cv_staged, cv_staged_room;
  std::deque<orcgpu_staged*> staged_q;        // staged, not yet decoded (stager -> decoder)
  int stager_rc = 0;                          // why the stager stopped early (0: it did not)
  std::string stager_err;
  std::deque<Ready> ready;                    // decoded, copy back under way (decoder -> caller)
  std::vector<orcgpu_result*> spare;          // results the caller is done with: their buffers are decoded into again
  bool worker_started = false, stager_done = false, worker_done = false, stop = false;
  bool has_predicate = false;                 // with_predicate
  std::vector<orcgpu_host::PredNode> predicate;
  // ---- row groups under a row selection (orcgpu_reader_set_row_group_pruning) ----
  bool prune = true;
  std::atomic<uint64_t> groups_read{0}, groups_total{0};
  std::deque<orcgpu_result*> serial_q;        // prefetch = 0: pieces of the current stripe decoded and not handed out yet
  // ---- row filter (orcgpu_reader_set_row_filter): the nodes as given, and -- from the first next_batch on -- their program ----
  bool has_filter = false, filter_ready = false, filter_failed = false;
  std::vector<orcgpu_host::PredNode> filter_nodes;
  orcgpu_host::FilterPlan filter_plan;
  std::atomic<uint64_t> filter_seen{0}, filter_kept{0};
  // ---- aggregates (orcgpu_reader_set_aggregates): the specs as given (their strings copied), and -- from orcgpu_reader_aggregate
  // on -- their instructions; every decoded stripe is aggregated where the filter and the copy back would stand ----
  bool has_aggs = false, aggs_done = false;
  struct AggSpec {
    uint32_t op = 0;
    bool has_column = false, has_column2 = false;
    std::string column, column2;
  };
  std::vector<AggSpec> agg_specs;
  orcgpu_host::AggPlan agg_plan;
  // ---- device output (orcgpu_reader_set_device_output): the batches are views of the results' HBM, handed out by
  // orcgpu_reader_next_batch_device; no copy back is started.  A result the caller is done with goes to `home` instead of `spare`
  // -- at once, or when the last exported batch or tensor that views it is released (device_hold.h) ----
  bool device_output = false;
  std::shared_ptr<orcgpu_hold::Home> home;
  uint64_t d2h_bytes = 0;                     // column-buffer bytes copied to the host so far (orcgpu_reader_d2h_bytes)
  bool current_counted = false;               // ... those of `current` are in it
  bool device_checked = false, device_refused = false;  // the projection has been looked at for nested columns; it has one
  std::string device_refused_name;
  const char* device_refused_kind = "";
};

static int arrow_code_of_format(const char* f, uint32_t* prec, uint32_t* scale);

namespace orcgpu_host {

int reader_build(orcgpu_reader* rd) {
  if (rd->built) return ORCGPU_OK;
  rd->built = true;
  rd->stripe_order.clear();
  for (size_t i = 0; i < rd->md.stripes.size(); i++) {
    uint64_t off = rd->md.stripes[i].offset;
    if (!rd->has_range || (off >= rd->range_start && off < rd->range_end)) rd->stripe_order.push_back(i);
  }
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
  // the projected root columns, in file order; with_schema: columns and fields are zipped (array_decoder/mod.rs:577-582): columns
  // beyond the schema's fields are not decoded
  std::vector<std::string> dict_seen;  // the dictionary columns (orcgpu_reader_set_dictionary_columns) met among the columns read
  std::vector<size_t> taken;
  for (size_t k = 0; k < root.subtypes.size(); k++) {
    const std::string nm = k < root.field_names.size() ? root.field_names[k] : std::string();
    const bool take = rd->project_all || (rd->by_index ? std::find(rd->projected_roots.begin(), rd->projected_roots.end(), (uint32_t)k) != rd->projected_roots.end()
                                                       : std::find(rd->projected_names.begin(), rd->projected_names.end(), nm) != rd->projected_names.end());
    if (!take) continue;
    if (rd->has_schema && taken.size() >= rd->schema_target.size()) break;
    taken.push_back(k);
  }
  // a column shard keeps this rank's share of them (orcgpu_reader_set_shard)
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
    // flat columns, and Structs of them (to any depth the decoder takes); List / Map / Union are not decoded on this path
    // `hint`: the Arrow field with_schema gives for this column (nullptr: none).  A nested column is matched with the nested Arrow
    // type of its kind and hands its children the fields below it, zipped by position (struct_decoder.rs:43-48, list.rs, map.rs,
    // union.rs); a pair that does not match is reported when the first stripe is planned, as MismatchedSchema.
    using SchemaNode = orcgpu_reader::SchemaNode;
    std::function<int(uint32_t, uint32_t, const std::string&, int, const SchemaNode*)> add = [&](uint32_t id, uint32_t parent, const std::string& field, int depth,
                                                                                               const SchemaNode* hint) -> int {
      if (id >= rd->md.types.size() || depth > kMaxTypeDepth) return ORCGPU_OUT_OF_SPEC;  // (a type tree cannot be deeper than it has types: a cycle)
      const OrcType& t = rd->md.types[id];
      const bool nested = t.kind == ORCGPU_T_STRUCT || t.kind == ORCGPU_T_LIST || t.kind == ORCGPU_T_MAP || t.kind == ORCGPU_T_UNION;
      if (!nested && !is_flat_kind(t.kind)) {
        set_err(rd->ctx, "column '%s': ORC type kind %d is not decoded on the GPU path", name.c_str(), t.kind);
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
          target = (hint->flags & 4) ? ORCGPU_ARROW_MAP_SORTED : ORCGPU_ARROW_MAP;  // ARROW_FLAG_MAP_KEYS_SORTED
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
    const size_t root_pos = ti;  // (position among the projected columns: the schema's field of the same position)
    rd->col_names.push_back(rd->has_schema ? rd->schema_names[root_pos] : name);
    int rc = add(cid, 0, std::string(), 0, rd->has_schema ? &rd->schema_tree[root_pos] : nullptr);
    if (rc) return rc;
  }
  // (every dictionary column must be among the columns read)
  for (auto& dn : rd->dict_names)
    if (std::find(dict_seen.begin(), dict_seen.end(), dn) == dict_seen.end() && rd->shard_mode != ORCGPU_SHARD_COLUMNS) {
      set_err(rd->ctx, "dictionary column '%s' is not among the projected columns", dn.c_str());
      return ORCGPU_INVALID_ARGUMENT;
    }
  return ORCGPU_OK;
}

// One stream of a stripe as it is read from the file: all of it, or from a row group's entry point on
struct StreamPiece {
  const StreamInfo* info;
  uint64_t start = 0, end = 0;  // bytes of the stream
  uint32_t skip_bytes = 0, skip_values = 0, skip_bits = 0;
  std::vector<orcgpu_stream_entry> entries;  // a whole stream: where its later row groups start, run starts for the walk (whole_stripe_entries)
};

// Stripe::new (stripe.rs:127-182): read (pieces of) the projected streams of a stripe and stage them in HBM (the copies are
// asynchronous: the decode waits for them on the device).
int reader_stage_rows(orcgpu_reader* rd, const StripeFooter& sf, const std::vector<StreamPiece>& pieces, uint64_t n_rows, orcgpu_staged** staged_out) {
  orcgpu_ctx* ctx = rd->ctx;
  std::vector<std::vector<uint8_t>> bufs;
  std::vector<orcgpu_stream> streams;
  bufs.reserve(pieces.size());
  for (auto& pc : pieces) {
    bufs.emplace_back();
    const uint8_t* where = rd->reader->view(pc.info->offset + pc.start, pc.end - pc.start);
    if (!where && !rd->reader->get_bytes(pc.info->offset + pc.start, pc.end - pc.start, bufs.back())) return ORCGPU_IO_ERROR;
    streams.push_back(orcgpu_stream{pc.info->column, pc.info->kind, where, pc.end - pc.start, pc.skip_bytes, pc.skip_values,
                                    pc.entries.empty() ? nullptr : pc.entries.data(), (uint32_t)pc.entries.size(), pc.skip_bits});
  }
  for (size_t i = 0; i < streams.size(); i++)
    if (!streams[i].ptr) streams[i].ptr = bufs[i].data();
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
    // (dictionary output: with_schema's field for such a column is Utf8, or there is no schema; any other field stays and mismatches)
    if (rd->col_dict[cols.size()] && (c.arrow_target == ORCGPU_ARROW_DEFAULT || c.arrow_target == ORCGPU_ARROW_UTF8)) c.arrow_target = ORCGPU_ARROW_DICTIONARY_UTF8;
    cols.push_back(c);
  }
  orcgpu_stripe_desc d{};
  d.n_rows = n_rows;
  d.compression = rd->md.compression;
  d.block_size = rd->md.block_size;
  d.ts_base_seconds = 1420070400;
  d.writer_timezone = sf.has_tz ? sf.writer_timezone.c_str() : nullptr;
  d.batch_size = rd->batch_size;
  d.n_streams = (uint32_t)streams.size();
  d.streams = streams.data();
  d.n_columns = (uint32_t)cols.size();
  d.columns = cols.data();
  return orcgpu_stage_stripe(ctx, &d, staged_out);  // (the caller's buffers may go as soon as it returns)
}

bool is_data_stream(const orcgpu_reader* rd, const StreamInfo& s) {
  if (std::find(rd->col_ids.begin(), rd->col_ids.end(), s.column) == rd->col_ids.end()) return false;
  return !(s.kind == ORCGPU_S_ROW_INDEX || s.kind == ORCGPU_S_BLOOM_FILTER || s.kind == ORCGPU_S_BLOOM_FILTER_UTF8 || s.kind == ORCGPU_S_DICTIONARY_COUNT);
}

// The row groups [g0, g1) of a stripe as stream pieces: every stream from the entry point its column's RowIndexEntry g0 names
// to where entry g1 points (and a little beyond: the run, or the chunks, that straddle the boundary).  false: the stripe's
// indexes cannot be used that way -- it is then decoded whole.
bool row_group_pieces(orcgpu_reader* rd, const StripeFooter& sf, uint64_t n_groups, uint64_t g0, uint64_t g1, std::vector<StreamPiece>& out) {
  const bool compressed = rd->md.compression != ORCGPU_COMP_NONE;
  out.clear();
  for (auto& s : sf.streams) {
    if (!is_data_stream(rd, s)) continue;
    StreamPiece pc;
    pc.info = &s;
    pc.end = s.length;
    const OrcType& t = rd->md.types[s.column];
    const int enc = s.column < sf.encodings.size() ? sf.encodings[s.column].first : 0;
    const bool dict_col = (t.kind == ORCGPU_T_STRING || t.kind == ORCGPU_T_VARCHAR || t.kind == ORCGPU_T_CHAR) &&
                          (enc == ORCGPU_ENC_DICTIONARY || enc == ORCGPU_ENC_DICTIONARY_V2);
    if (s.kind == ORCGPU_S_DICTIONARY_DATA || (dict_col && s.kind == ORCGPU_S_LENGTH)) {  // dictionaries: whole
      out.push_back(pc);
      continue;
    }
    // (List / Map: their LENGTH stream is entered like any RLE stream, and their elements' streams at the positions the
    // elements' own index entries hold for the same row group -- how many elements a piece has follows from its lengths, as in a
    // whole stripe.  A Union (round 6): its tags -- byte RLE -- are entered like any run-length stream, and every arm's child at the
    // positions the CHILD's own index entries hold for the row group: a writer records, at every row-group boundary, how far each
    // column's streams have got, an arm's child included -- its count is the rows whose tag named it so far.  How many values of
    // an arm a piece holds follows from the piece's tags, as in a whole stripe (union.rs:69-136).)
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
      // a run holds at most 512 values; a chunk at most block_size bytes; a bit stream may be entered in mid-byte (round 5)
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
        // the chunk the boundary lies in and the one behind it (a run may straddle two chunks; a writer's chunks are full blocks but
        // for the last of a stream): their 3-byte headers say where they end
        for (int k = 0; k < 2 && end < s.length; k++) {
          std::vector<uint8_t> h;
          if (s.length - end < 3 || !rd->reader->get_bytes(s.offset + end, 3, h)) return false;
          const uint64_t len = ((uint64_t)h[0] | ((uint64_t)h[1] << 8) | ((uint64_t)h[2] << 16)) >> 1;
          if (len > s.length - end - 3) return false;
          end += 3 + len;
        }
      } else {
        end = std::min<uint64_t>(s.length, end + 8192);  // (the longest run: 512 values of 8 bytes, its header and patch list)
      }
      pc.end = end;
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
void whole_stripe_entries(orcgpu_reader* rd, const StripeFooter& sf, uint64_t n_groups, std::vector<StreamPiece>& whole) {
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
    // (a lane per entry follows its row group's runs one memory round trip at a time: worth it where the runs are long -- streams
    // of 16 KiB or more per row group --, not for the thousands of short runs of a narrow stream, which the span walk finds
    // faster by itself: with the positions of every stream a 24 M-row lineitem file read 8 ms slower)
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

// The next stripe of the file -> staged rows: the whole stripe, or -- under a row selection, when its ROW_INDEX streams allow
// it -- one staged piece per run of consecutive row groups that hold selected rows (none: the stripe is not read at all).
int reader_stage_next(orcgpu_reader* rd, std::vector<orcgpu_staged*>& out) {
  orcgpu_ctx* ctx = rd->ctx;
  const size_t at = rd->next_stripe++;
  const StripeInfo& si = rd->md.stripes[rd->stripe_order[at]];
  if (rd->shard_world > 1 && rd->shard_mode == ORCGPU_SHARD_STRIPES && at % rd->shard_world != rd->shard_rank) {
    // another rank's stripe: it still takes its share of the row selection (arrow_reader.rs:296-308), nothing of it is read
    if (rd->has_selection && sel_row_count(rd->selection) > 0) (void)sel_split_off(rd->selection, si.number_of_rows);
    return ORCGPU_OK;
  }
  StripeFooter local;
  int rc = 0;
  if (at >= rd->footers.size()) {
    if (rd->footers_read) {  // (read-ahead: this footer is the one that could not be read)
      set_err(ctx, "%s", rd->footers_err.c_str());
      return rd->footers_rc ? rd->footers_rc : ORCGPU_UNEXPECTED;
    }
    rc = read_stripe_footer(ctx, *rd->reader, rd->md, si, local);
  }
  if (rc) return rc;
  StripeFooter& sf = at < rd->footers.size() ? rd->footers[at] : local;
  const uint64_t n_rows = si.number_of_rows;
  // arrow_reader.rs:296-308: the stripe takes its share of the selection; with no rows left in it, stripes are read whole
  bool has_sel = false;
  std::vector<SelBatch> batches;
  std::vector<RowSel> mine;
  const uint64_t stride = rd->md.row_index_stride;
  if (rd->has_predicate) {
    // arrow_reader.rs:258-293: the predicate against the stripe's row indexes -> the row groups to keep -> a RowSelection
    // (from_row_group_filter, row_selection.rs:348-392: rows_per_group rows per kept / skipped group, neighbours merged); an
    // evaluation that fails selects every row
    if (!sf.index_read && read_stripe_index(ctx, *rd->reader, rd->md, sf, rd->col_ids, true)) sf.index.clear();
    std::vector<std::string> names;
    std::vector<ColumnGroups> cols;
    for (size_t k = 0, root = 0; k < rd->col_ids.size(); k++) {
      if (rd->col_parent[k]) continue;
      const std::string& name = rd->col_names[root++];
      for (auto& ci : sf.index)
        if (ci.column == rd->col_ids[k] && ci.has_groups) {
          names.push_back(name);
          cols.push_back(ci.groups);
        }
    }
    std::vector<uint8_t> keep;
    const uint64_t ng = stride ? (n_rows + stride - 1) / stride : 0;
    if (predicate_row_groups(rd->predicate, names, cols, (size_t)ng, keep)) {
      if (keep.empty()) mine.push_back(RowSel{n_rows, true});  // RowSelection::skip_all
      for (uint8_t k : keep) {
        if (!mine.empty() && mine.back().skip == !k) mine.back().row_count += stride;
        else mine.push_back(RowSel{stride, !k});
      }
    } else {
      mine.push_back(RowSel{n_rows, false});  // RowSelection::select_all
    }
    has_sel = true;
  }
  if (rd->has_selection && sel_row_count(rd->selection) > 0) {
    std::vector<RowSel> share = sel_split_off(rd->selection, n_rows);
    mine = has_sel ? sel_intersect(share, mine, n_rows) : share;
    has_sel = true;
  }
  if (has_sel) batches = sel_batches(mine, n_rows, rd->batch_size);
  const uint64_t n_groups = stride ? (n_rows + stride - 1) / stride : 1;
  rd->groups_total += n_groups;
  std::vector<StreamPiece> whole;
  for (auto& s : sf.streams)
    if (is_data_stream(rd, s)) {
      StreamPiece pc;
      pc.info = &s;
      pc.end = s.length;
      whole.push_back(pc);
    }
  if (has_sel && rd->prune) {
    if (batches.empty()) return ORCGPU_OK;  // nothing of the stripe is selected: not read
    if (stride && n_groups > 1) {
      if (!sf.index_read) {
        if (read_stripe_index(ctx, *rd->reader, rd->md, sf, rd->col_ids, false)) sf.index.clear();  // (an index that cannot be read: the stripe is decoded whole)
      }
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
      if (rd->has_filter && ranges.size() > 1) ranges = {{ranges.front().first, ranges.back().second}};
      std::vector<std::vector<StreamPiece>> pieces(ranges.size());
      bool usable = !(ranges.size() == 1 && ranges[0].first == 0 && ranges[0].second == n_groups);
      for (size_t k = 0; k < ranges.size() && usable; k++) usable = row_group_pieces(rd, sf, n_groups, ranges[k].first, ranges[k].second, pieces[k]);
      if (usable) {
        for (size_t k = 0; k < ranges.size(); k++) {
          const uint64_t r0 = ranges[k].first * stride, r1 = std::min<uint64_t>(n_rows, ranges[k].second * stride);
          orcgpu_staged* st = nullptr;
          rc = reader_stage_rows(rd, sf, pieces[k], r1 - r0, &st);
          if (rc) return rc;
          st->has_sel = true;
          st->piece = true;
          for (auto& b : batches)
            if (b.start >= r0 && b.start < r1) st->sel.push_back(SelBatch{b.start - r0, b.len, 0});
          rd->groups_read += ranges[k].second - ranges[k].first;
          out.push_back(st);
        }
        return ORCGPU_OK;
      }
    }
  }
  constexpr bool no_entries = false;
  if (sf.index_read && stride && !no_entries) whole_stripe_entries(rd, sf, n_groups, whole);
  orcgpu_staged* st = nullptr;
  rc = reader_stage_rows(rd, sf, whole, n_rows, &st);
  if (rc) return rc;
  // (a selection that asks for every row in the batches the stripe has anyway -- a predicate that keeps all row groups -- is none)
  bool as_decoded = has_sel && rd->batch_size && batches.size() == (n_rows + rd->batch_size - 1) / rd->batch_size;
  for (size_t k = 0; k < batches.size() && as_decoded; k++)
    as_decoded = batches[k].start == (uint64_t)k * rd->batch_size && batches[k].len == std::min<uint64_t>(rd->batch_size, n_rows - batches[k].start);
  st->has_sel = has_sel && !as_decoded;
  if (st->has_sel) st->sel = std::move(batches);
  rd->groups_read += n_groups;
  out.push_back(st);
  return ORCGPU_OK;
}

// Every stripe footer of the file -- and, under a predicate or a row selection, the row indexes the stripes will be asked for --
// read now, by one call of the GPU decompressors each (rather than one or two calls per stripe as their turns come).
void reader_read_metadata_ahead(orcgpu_reader* rd) {
  auto owned = [rd](size_t at) { return !(rd->shard_world > 1 && rd->shard_mode == ORCGPU_SHARD_STRIPES && at % rd->shard_world != rd->shard_rank); };
  const size_t n = rd->stripe_order.size();
  std::vector<const StripeInfo*> infos;
  std::vector<size_t> at_of;
  for (size_t k = 0; k < n; k++)
    if (owned(k)) {  // (another rank's stripe: nothing of it is read, not its footer either)
      infos.push_back(&rd->md.stripes[rd->stripe_order[k]]);
      at_of.push_back(k);
    }
  std::vector<StripeFooter> got;
  const size_t n_read = read_stripe_footers(rd->ctx, *rd->reader, rd->md, infos, got, &rd->footers_rc);
  // (a footer that cannot be read: the stripes before it are still handed out, the error arrives in its place)
  const size_t n_upto = n_read < infos.size() ? at_of[n_read] : n;
  if (n_read < infos.size()) rd->footers_err = rd->ctx->err;
  rd->footers.assign(n_upto, StripeFooter{});
  for (size_t k = 0; k < n_read; k++) rd->footers[at_of[k]] = std::move(got[k]);
  std::vector<StripeFooter*> want;
  if (rd->has_predicate) {
    // ... and so are the row indexes (statistics, Bloom filters, positions) of every stripe, for the predicate
    for (size_t k = 0; k < n_upto; k++)
      if (owned(k)) want.push_back(&rd->footers[k]);
    read_stripe_indexes(rd->ctx, *rd->reader, rd->md, want, rd->col_ids, true);
  } else if (rd->has_selection && rd->prune && rd->md.row_index_stride) {
    // ... and so are the ROW_INDEX streams of the stripes that hold selected rows (the selection is stepped through once, dry)
    std::vector<RowSel> sel = rd->selection;
    for (size_t k = 0; k < n_upto; k++) {
      const uint64_t n_rows = rd->md.stripes[rd->stripe_order[k]].number_of_rows;
      if (!sel_row_count(sel)) break;
      std::vector<RowSel> mine = sel_split_off(sel, n_rows);
      if (!owned(k) || n_rows <= rd->md.row_index_stride || sel_batches(mine, n_rows, rd->batch_size).empty()) continue;
      want.push_back(&rd->footers[k]);
    }
    read_stripe_indexes(rd->ctx, *rd->reader, rd->md, want, rd->col_ids, false);
  }
  rd->footers_read = true;
}

// The row filter on one decoded (and selected) stripe.  A stripe whose decode failed is left as it is: its error arrives with
// its failing batch.
int reader_filter_result(orcgpu_reader* rd, orcgpu_result* res) {
  if (res->status) return ORCGPU_OK;
  uint64_t seen = 0, kept = 0;
  const int rc = result_filter_plan(rd->ctx, res, rd->filter_plan, &seen, &kept);
  rd->filter_seen += seen;
  rd->filter_kept += kept;
  return rc;
}

// The filter's nodes against the projected root columns -> its program, once, at the first next_batch
int reader_compile_filter(orcgpu_reader* rd) {
  std::vector<const char*> names;
  std::vector<int32_t> kinds, params;
  for (size_t k = 0, root = 0; k < rd->col_ids.size(); k++) {
    // (a column below a Struct / List / Map / Union: its root is refused by its kind)
    if (rd->col_parent[k]) continue;
    const OrcType& t = rd->md.types[rd->col_ids[k]];
    names.push_back(rd->col_names[root++].c_str());
    kinds.push_back(t.kind);
    // what a Decimal128 / TimestampNs literal is brought to: the column's scale (with_schema takes no other), the unit it is decoded to
    orcgpu_column c{};
    c.arrow_target = rd->has_schema ? rd->col_target[k] : rd->ts_arrow_target;
    params.push_back(t.kind == ORCGPU_T_DECIMAL ? (int32_t)t.scale : ts_unit_of(c));
  }
  const std::vector<orcgpu_predicate_node> nodes = view_predicate(rd->filter_nodes);
  const int rc = filter_compile(nodes.data(), (uint32_t)nodes.size(), names.data(), kinds.data(), (uint32_t)names.size(), rd->filter_plan, params.data());
  if (rc) set_err(rd->ctx, "%s", rd->filter_plan.err);
  if (rc) return rc;
  // a comparison on a dictionary-output column would have to be evaluated on the entries: refused, by name, before anything is read
  for (auto& in : rd->filter_plan.prog) {
    if (!fop_reads_values(in.op) || in.col >= names.size()) continue;
    size_t root = 0;
    for (size_t k = 0; k < rd->col_ids.size(); k++) {
      if (rd->col_parent[k]) continue;
      if (root++ == in.col && rd->col_dict[k]) {
        set_err(rd->ctx, "row filter: column '%s' is read as a dictionary column (orcgpu_reader_set_dictionary_columns): a comparison on it is not supported", names[in.col]);
        return ORCGPU_UNSUPPORTED;
      }
    }
  }
  return ORCGPU_OK;
}

std::vector<orcgpu_agg_spec> reader_view_aggs(const orcgpu_reader* rd) {
  std::vector<orcgpu_agg_spec> out(rd->agg_specs.size());
  for (size_t k = 0; k < out.size(); k++) {
    const orcgpu_reader::AggSpec& s = rd->agg_specs[k];
    out[k] = {s.op, s.has_column ? s.column.c_str() : nullptr, s.has_column2 ? s.column2.c_str() : nullptr};
  }
  return out;
}

// The aggregate list against the projected root columns as the file's metadata and the builder describe them -> its instructions,
// once, before anything is read: every refusal arrives here.  (What a stripe's decode made of the columns is checked again, per
// stripe, by the plan the kernels run: reader_aggregate_result.)
int reader_compile_aggs(orcgpu_reader* rd) {
  std::vector<const char*> names;
  std::vector<AggCol> cols;
  for (size_t k = 0, root = 0; k < rd->col_ids.size(); k++) {
    if (rd->col_parent[k]) continue;
    const OrcType& t = rd->md.types[rd->col_ids[k]];
    names.push_back(rd->col_names[root++].c_str());
    orcgpu_column c{};
    c.arrow_target = rd->has_schema ? rd->col_target[k] : rd->ts_arrow_target;
    AggCol a;
    a.d.orc_type = t.kind;
    a.d.ts_unit = ts_unit_of(c);
    a.d.is_bool = t.kind == ORCGPU_T_BOOLEAN;
    a.d.dict_out = rd->col_dict[k] != 0;
    a.d.is_string = !a.d.dict_out && (t.kind == ORCGPU_T_STRING || t.kind == ORCGPU_T_VARCHAR || t.kind == ORCGPU_T_CHAR || t.kind == ORCGPU_T_BINARY);
    const bool is_ts = t.kind == ORCGPU_T_TIMESTAMP || t.kind == ORCGPU_T_TIMESTAMP_INSTANT;
    a.d.width = t.kind == ORCGPU_T_BYTE ? 1 : t.kind == ORCGPU_T_SHORT ? 2 : (t.kind == ORCGPU_T_INT || t.kind == ORCGPU_T_FLOAT || t.kind == ORCGPU_T_DATE || a.d.dict_out) ? 4
                : (t.kind == ORCGPU_T_DECIMAL || (is_ts && a.d.ts_unit > 3)) ? 16 : (a.d.is_bool || a.d.is_string) ? 0 : 8;
    a.scale = t.scale;
    a.nested = t.kind == ORCGPU_T_STRUCT || t.kind == ORCGPU_T_LIST || t.kind == ORCGPU_T_MAP || t.kind == ORCGPU_T_UNION;
    cols.push_back(a);
  }
  const std::vector<orcgpu_agg_spec> specs = reader_view_aggs(rd);
  const int rc = agg_compile(specs.data(), (uint32_t)specs.size(), names.data(), cols.data(), (uint32_t)cols.size(), rd->agg_plan);
  if (rc) set_err(rd->ctx, "%s", rd->agg_plan.err);
  return rc;
}

// The aggregation of one decoded (and selected) stripe, where reader_filter_result and the copy back stand otherwise: its
// records stay with the result until orcgpu_reader_aggregate merges them, in stripe order.  A stripe whose decode failed ends the call.
int reader_aggregate_result(orcgpu_reader* rd, orcgpu_result* res) {
  if (res->status) {
    set_err(rd->ctx, "stripe decode failed in batch %u, column %u", res->err_batch, res->err_col);
    return res->status;
  }
  std::vector<const char*> names;
  for (auto& n : rd->col_names) names.push_back(n.c_str());
  if (names.size() != res->cols.size()) {  // (a flat projection: one result column per root column; anything else the plan has refused)
    set_err(rd->ctx, "aggregate: the result holds %zu columns for %zu projected root columns", res->cols.size(), names.size());
    return ORCGPU_UNSUPPORTED;
  }
  const std::vector<orcgpu_agg_spec> specs = reader_view_aggs(rd);
  AggPlan plan;
  if (const int rc = result_compile_aggs(rd->ctx, res, specs.data(), (uint32_t)specs.size(), names.data(), plan)) return rc;
  for (size_t k = 0; k < plan.insns.size(); k++)
    if (plan.insns[k].kind != rd->agg_plan.insns[k].kind || plan.insns[k].scale != rd->agg_plan.insns[k].scale) {
      set_err(rd->ctx, "aggregate: column '%s' is not decoded to the type its aggregate was planned for", names[plan.insns[k].col]);
      return ORCGPU_MISMATCHED_SCHEMA;
    }
  const int rc = result_aggregate_plan(rd->ctx, res, rd->has_filter ? &rd->filter_plan : nullptr, plan, res->agg_records, &res->agg_seen, names.data(), (uint32_t)names.size());
  if (rc) return rc;
  rd->filter_seen += res->agg_seen;
  rd->filter_kept += res->agg_records.back().w[0];
  return ORCGPU_OK;
}

// A result the caller is done with, to decode a later stripe into (rd->m is held by a reader that reads ahead)
orcgpu_result* reader_take_spare(orcgpu_reader* rd) {
  // (a result that comes home was viewed by batches and tensors whose consumers released them on the HOST: work they enqueued on
  // streams of their own may not have run yet, and nothing orders the decode stream behind it -- so decode_staged_once waits for
  // the device before it writes into a result that has been exported)
  if (rd->device_output && !rd->has_aggs) return static_cast<orcgpu_result*>(orcgpu_hold::home_take(*rd->home));
  if (rd->spare.empty()) return nullptr;
  orcgpu_result* r = rd->spare.back();
  rd->spare.pop_back();
  return r;
}
void reader_give_spare(orcgpu_reader* rd, orcgpu_result* r) {
  if (rd->device_output && r->hold) orcgpu_hold::hold_owner_done(r->hold, true);  // (now, or when its last exported batch is released)
  else rd->spare.push_back(r);
}
// A decoded stripe on its way to the caller: the host path starts its copy back, the device path adopts it (its references are
// counted from here on, its home is this reader) and marks where on the decode stream it is complete
int reader_result_decoded(orcgpu_reader* rd, orcgpu_result* r, bool start_copy) {
  if (!rd->device_output) return start_copy ? orcgpu_result_fetch_async(rd->ctx, r) : ORCGPU_OK;
  if (!r->hold) r->hold = orcgpu_hold::hold_new(r, result_destroy, rd->home);
  return result_mark_ready(rd->ctx, r);
}

// prefetch = 0: both steps in the caller's thread (the pieces of a stripe in one decode call).  ORCGPU_END_OF_FILE = the file has no more rows to give
int reader_advance_stripe(orcgpu_reader* rd) {
  orcgpu_ctx* ctx = rd->ctx;
  while (rd->serial_q.empty()) {
    if (rd->next_stripe >= rd->stripe_order.size()) return ORCGPU_END_OF_FILE;
    const bool host_prof = getenv("ORCGPU_DEBUG") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    if (!rd->footers_read) reader_read_metadata_ahead(rd);
    const double t1 = now();
    // a stripe -- or, when a selection leaves little of them, the pieces of several: a decode call costs its longest block
    // chain (milliseconds) however little it decodes, so small pieces share one
    std::vector<orcgpu_staged*> got;
    int rc = 0;
    uint64_t staged_bytes = 0;
    do {
      const size_t before = got.size();
      rc = reader_stage_next(rd, got);
      for (size_t k = before; k < got.size(); k++) staged_bytes += orcgpu_staged_bytes(got[k]);
    } while (!rc && rd->next_stripe < rd->stripe_order.size() && got.size() < 32 && staged_bytes < (64u << 20));
    std::vector<orcgpu_result*> res(got.size(), nullptr);
    for (auto& r : res) r = reader_take_spare(rd);  // (results the caller is done with are decoded into again: their arenas and pinned host copies stay)
    const double t2 = now();
    if (!rc && !got.empty()) rc = orcgpu_decode_staged(ctx, got.data(), (uint32_t)got.size(), res.data());
    const double t3 = now();
    for (size_t k = 0; k < got.size(); k++) {
      if (!rc) res[k]->field_names = rd->col_field;
      if (!rc && got[k]->has_sel) rc = result_select_batches(ctx, res[k], got[k]->sel);  // (the stripe's share of the selection)
      if (!rc && rd->has_aggs) rc = reader_aggregate_result(rd, res[k]);  // (in place of the filter's compaction and of any copy back)
      else if (!rc && rd->has_filter) rc = reader_filter_result(rd, res[k]);
      orcgpu_staged_free(got[k]);
      if (!rc && !rd->has_aggs) rc = reader_result_decoded(rd, res[k], false);  // (the host path copies back when the first batch is asked for)
    }
    if (host_prof)
      fprintf(stderr, "[orcgpu] reader: metadata %.2f ms, staging %zu pieces (%.1f MB) %.2f ms, decode %.2f ms, selection %.2f ms\n", t1 - t0,
              got.size(), staged_bytes / 1e6, t2 - t1, t3 - t2, now() - t3);
    if (rc) {
      for (auto* r : res)
        if (r) orcgpu_result_free(r);
      return rc;
    }
    for (auto* r : res) rd->serial_q.push_back(r);
  }
  if (rd->current) reader_give_spare(rd, rd->current);
  rd->current = rd->serial_q.front();
  rd->serial_q.pop_front();
  rd->next_batch = 0;
  rd->current_counted = false;
  return ORCGPU_OK;
}

uint64_t staged_queue_bytes(const orcgpu_reader* rd) {
  uint64_t b = 0;
  for (auto* st : rd->staged_q) b += orcgpu_staged_bytes(st);
  return b;
}

// The stager of a reading-ahead reader (see orcgpu_reader): file bytes -> HBM, up to 2 x prefetch stripes ahead of the decoder.
void reader_stager(orcgpu_reader* rd) {
  (void)hipSetDevice(rd->ctx->device);
  int rc = 0;
  while (!rc && rd->next_stripe < rd->stripe_order.size()) {
    {
      std::unique_lock<std::mutex> g(rd->m);
      // (small pieces -- what a selection leaves of its stripes -- queue up beyond that: they are decoded many to a call)
      rd->cv_staged_room.wait(g, [rd] {
        if (rd->stop || rd->staged_q.size() < 2 * (size_t)rd->prefetch) return true;
        return rd->staged_q.size() < 32 && staged_queue_bytes(rd) < (64u << 20);
      });
      if (rd->stop) break;
    }
    std::vector<orcgpu_staged*> got;
    rc = reader_stage_next(rd, got);
    {
      std::lock_guard<std::mutex> g(rd->m);
      for (auto* st : got) rd->staged_q.push_back(st);
    }
    if (rc) break;
    rd->cv_staged.notify_all();
  }
  {
    std::lock_guard<std::mutex> g(rd->m);
    rd->stager_rc = rc;
    if (rc) rd->stager_err = rd->ctx->err;
    rd->stager_done = true;
  }
  rd->cv_staged.notify_all();
}

// ... and its decoder: the stripes staged so far (at most as many as the caller has room for) in ONE decode call, the stripe's
// share of the row selection, the copies back started, the results queued in file order.
void reader_decoder(orcgpu_reader* rd) {
  orcgpu_ctx* ctx = rd->ctx;
  (void)hipSetDevice(ctx->device);
  int rc = 0;
  std::string err;
  for (;;) {
    std::vector<orcgpu_staged*> group;
    std::vector<orcgpu_result*> results;
    {
      std::unique_lock<std::mutex> g(rd->m);
      rd->cv_room.wait(g, [rd] { return rd->stop || rd->ready.size() < rd->prefetch; });
      if (rd->stop) break;
      // (a decode call costs its launch chain however little it decodes: a few small pieces wait for the ones being staged)
      // -- pieces of stripes for all the others, up to what one call takes: 1 % of a file's row groups is then ONE call
      rd->cv_staged.wait(g, [rd] {
        if (rd->stop || rd->stager_done) return true;
        if (rd->staged_q.empty()) return false;
        bool pieces_only = true;
        for (auto* st : rd->staged_q) pieces_only = pieces_only && st->piece;
        return rd->staged_q.size() >= 32 || staged_queue_bytes(rd) >= (pieces_only ? (48u << 20) : (8u << 20));
      });
      if (rd->stop) break;
      if (rd->staged_q.empty()) {  // the stager is done: the end of the file, or its error
        rc = rd->stager_rc;
        err = rd->stager_err;
        break;
      }
      // as many as the caller has room for -- and small pieces (what a selection leaves of its stripes) eight at a time whatever
      // the room: a decode call costs its longest block chain however little it decodes
      const size_t room = rd->prefetch - rd->ready.size();
      uint64_t group_bytes = 0;
      while (!rd->staged_q.empty() && group.size() < 32 &&
             (group.size() < room || group_bytes + orcgpu_staged_bytes(rd->staged_q.front()) <= (64u << 20))) {
        group_bytes += orcgpu_staged_bytes(rd->staged_q.front());
        group.push_back(rd->staged_q.front());
        rd->staged_q.pop_front();
        results.push_back(reader_take_spare(rd));  // (a result the caller has given back is decoded into again: no allocations in steady state)
      }
    }
    rd->cv_staged_room.notify_all();
    rc = orcgpu_decode_staged(ctx, group.data(), (uint32_t)group.size(), results.data());
    for (size_t k = 0; k < group.size(); k++) {
      if (!rc) results[k]->field_names = rd->col_field;
      if (!rc && group[k]->has_sel) rc = result_select_batches(ctx, results[k], group[k]->sel);  // (the stripe's share of the selection)
      if (!rc && rd->has_aggs) rc = reader_aggregate_result(rd, results[k]);  // (in place of the filter's compaction and of the copy back)
      else if (!rc && rd->has_filter) rc = reader_filter_result(rd, results[k]);  // (before the copy back is started: only the kept rows cross the link)
      orcgpu_staged_free(group[k]);
      if (!rc && !rd->has_aggs) rc = reader_result_decoded(rd, results[k], true);
    }
    if (rc) {
      err = ctx->err;
      for (auto* r : results)
        if (r) orcgpu_result_free(r);
      break;
    }
    {
      std::lock_guard<std::mutex> g(rd->m);
      for (auto* r : results) {
        orcgpu_reader::Ready item;
        item.res = r;
        rd->ready.push_back(std::move(item));
      }
    }
    rd->cv_ready.notify_all();
  }
  {
    std::lock_guard<std::mutex> g(rd->m);
    if (rc) {
      orcgpu_reader::Ready item;
      item.rc = rc;
      item.err = err;
      rd->ready.push_back(std::move(item));
    }
    rd->worker_done = true;
  }
  rd->cv_ready.notify_all();
}

void reader_stop_worker(orcgpu_reader* rd) {
  if (!rd->worker_started) return;
  {
    std::lock_guard<std::mutex> g(rd->m);
    rd->stop = true;
  }
  rd->cv_room.notify_all();
  rd->cv_staged.notify_all();
  rd->cv_staged_room.notify_all();
  if (rd->stager.joinable()) rd->stager.join();
  if (rd->decoder.joinable()) rd->decoder.join();
  for (auto* st : rd->staged_q) orcgpu_staged_free(st);
  rd->staged_q.clear();
  for (auto& it : rd->ready)
    if (it.res) orcgpu_result_free(it.res);
  rd->ready.clear();
  for (auto* r : rd->spare) orcgpu_result_free(r);
  rd->spare.clear();
}

}  // namespace orcgpu_host

extern "C" {

static int reader_open_common(orcgpu_ctx* ctx, std::unique_ptr<orcgpu_host::ChunkReader> r, orcgpu_reader** out) {
  orcgpu_reader* rd = new orcgpu_reader();
  rd->ctx = ctx;
  rd->reader = std::move(r);
  int rc = orcgpu_host::read_metadata(ctx, *rd->reader, rd->md);
  if (rc) {
    delete rd;
    return rc;
  }
  *out = rd;
  return ORCGPU_OK;
}

int orcgpu_reader_open_file(orcgpu_ctx* ctx, const char* path, orcgpu_reader** out) {
  if (!ctx || !path || !out) return ORCGPU_INVALID_ARGUMENT;
  auto r = std::make_unique<orcgpu_host::FileChunkReader>(path);
  if (!r->f) {
    set_err(ctx, "cannot open '%s'", path);
    return ORCGPU_IO_ERROR;
  }
  return reader_open_common(ctx, std::move(r), out);
}
int orcgpu_reader_open_bytes(orcgpu_ctx* ctx, const uint8_t* data, uint64_t len, orcgpu_reader** out) {
  if (!ctx || (!data && len) || !out) return ORCGPU_INVALID_ARGUMENT;
  return reader_open_common(ctx, std::make_unique<orcgpu_host::BytesChunkReader>(data, len), out);
}
void orcgpu_reader_close(orcgpu_reader* rd) {
  if (!rd) return;
  orcgpu_host::reader_stop_worker(rd);
  if (rd->current) orcgpu_result_free(rd->current);
  for (auto* r : rd->serial_q) orcgpu_result_free(r);
  for (auto* r : rd->spare) orcgpu_result_free(r);
  rd->spare.clear();
  // (results that exported device batches still view are freed by the last of them: nothing comes home from here on)
  if (rd->home)
    for (void* r : orcgpu_hold::home_close(*rd->home)) orcgpu_result_free(static_cast<orcgpu_result*>(r));
  delete rd;
}
int orcgpu_reader_set_predicate(orcgpu_reader* rd, const orcgpu_predicate_node* nodes, uint32_t n_nodes) {
  if (!rd || rd->built || !nodes || !n_nodes) return ORCGPU_INVALID_ARGUMENT;
  rd->predicate = orcgpu_host::copy_predicate(nodes, n_nodes);
  rd->has_predicate = true;
  return ORCGPU_OK;
}
int orcgpu_reader_set_row_filter(orcgpu_reader* rd, const orcgpu_predicate_node* nodes, uint32_t n_nodes) {
  if (!rd || rd->built || !nodes || !n_nodes) return ORCGPU_INVALID_ARGUMENT;
  rd->filter_nodes = orcgpu_host::copy_predicate(nodes, n_nodes);
  rd->has_filter = true;
  return ORCGPU_OK;
}
int orcgpu_reader_filter_rows(const orcgpu_reader* rd, uint64_t* rows_seen, uint64_t* rows_kept) {
  if (!rd) return ORCGPU_INVALID_ARGUMENT;
  if (rows_seen) *rows_seen = rd->filter_seen.load();
  if (rows_kept) *rows_kept = rd->filter_kept.load();
  return ORCGPU_OK;
}
int orcgpu_reader_set_row_group_pruning(orcgpu_reader* rd, int on) {
  if (!rd || rd->built) return ORCGPU_INVALID_ARGUMENT;
  rd->prune = on != 0;
  return ORCGPU_OK;
}
int orcgpu_reader_row_groups(const orcgpu_reader* rd, uint64_t* read, uint64_t* total) {
  if (!rd) return ORCGPU_INVALID_ARGUMENT;
  if (read) *read = rd->groups_read.load();
  if (total) *total = rd->groups_total.load();
  return ORCGPU_OK;
}
int orcgpu_reader_set_prefetch(orcgpu_reader* rd, uint32_t stripes) {
  if (!rd || rd->built) return ORCGPU_INVALID_ARGUMENT;
  rd->prefetch = stripes > 8 ? 8 : stripes;
  return ORCGPU_OK;
}
int orcgpu_reader_set_batch_size(orcgpu_reader* rd, uint32_t n) {
  if (!rd || !n || rd->built) return ORCGPU_INVALID_ARGUMENT;
  rd->batch_size = n;
  return ORCGPU_OK;
}
int orcgpu_reader_set_projection(orcgpu_reader* rd, const char* const* names, uint32_t n) {
  if (!rd || rd->built) return ORCGPU_INVALID_ARGUMENT;
  rd->project_all = false;
  rd->projected_names.clear();
  for (uint32_t i = 0; i < n; i++) rd->projected_names.emplace_back(names[i]);
  return ORCGPU_OK;
}
int orcgpu_reader_set_dictionary_columns(orcgpu_reader* rd, const char* const* names, uint32_t n) {
  if (!rd || rd->built || (n && !names)) return ORCGPU_INVALID_ARGUMENT;
  std::vector<std::string> list;
  int rc = ORCGPU_OK;
  if (n) {
    char msg[256] = "";
    std::vector<std::string> roots;
    std::vector<int32_t> kinds;
    if (!rd->md.types.empty()) {
      const orcgpu_host::OrcType& root = rd->md.types[0];
      for (size_t k = 0; k < root.subtypes.size(); k++) {
        roots.push_back(k < root.field_names.size() ? root.field_names[k] : std::string());
        kinds.push_back(root.subtypes[k] < rd->md.types.size() ? rd->md.types[root.subtypes[k]].kind : -1);
      }
    }
    std::vector<const char*> rp;
    for (auto& s : roots) rp.push_back(s.c_str());
    rc = orcgpu_host::check_dictionary_names(names, n, rp.data(), kinds.data(), (uint32_t)rp.size(), msg, sizeof(msg));
    if (rc) {
      set_err(rd->ctx, "%s", msg);
      return rc;
    }
    for (uint32_t i = 0; i < n; i++) list.emplace_back(names[i]);
  }
  rd->dict_names.swap(list);
  return ORCGPU_OK;
}
int orcgpu_reader_set_projection_roots(orcgpu_reader* rd, const uint32_t* roots, uint32_t n) {
  if (!rd || rd->built || (n && !roots)) return ORCGPU_INVALID_ARGUMENT;
  rd->project_all = false;
  rd->by_index = true;
  rd->projected_roots.assign(roots, roots + n);
  return ORCGPU_OK;
}
// Arrow C Data Interface format string of a field -> ORCGPU_ARROW_* (+ precision / scale)
static int arrow_code_of_format(const char* f, uint32_t* prec, uint32_t* scale) {
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
int orcgpu_reader_set_schema(orcgpu_reader* rd, const struct ArrowSchema* schema) {
  if (!rd || rd->built || !schema || !schema->format || strcmp(schema->format, "+s") != 0) return ORCGPU_INVALID_ARGUMENT;
  rd->has_schema = true;
  rd->schema_target.clear();
  rd->schema_precision.clear();
  rd->schema_scale.clear();
  rd->schema_names.clear();
  rd->schema_tree.clear();
  std::function<void(const ArrowSchema*, orcgpu_reader::SchemaNode&)> walk = [&](const ArrowSchema* c, orcgpu_reader::SchemaNode& nd) {
    nd.format = c && c->format ? c->format : "";
    nd.name = c && c->name ? c->name : "";
    nd.flags = c ? c->flags : 0;
    if (c)
      for (int64_t k = 0; k < c->n_children; k++) {
        nd.kids.emplace_back();
        walk(c->children[k], nd.kids.back());
      }
  };
  for (int64_t i = 0; i < schema->n_children; i++) {
    const ArrowSchema* c = schema->children[i];
    uint32_t p = 0, sc = 0;
    rd->schema_target.push_back(arrow_code_of_format(c ? c->format : nullptr, &p, &sc));
    rd->schema_precision.push_back(p);
    rd->schema_scale.push_back(sc);
    rd->schema_names.emplace_back(c && c->name ? c->name : "");
    rd->schema_tree.emplace_back();
    walk(c, rd->schema_tree.back());
  }
  return ORCGPU_OK;
}
int orcgpu_reader_set_shard(orcgpu_reader* rd, uint32_t rank, uint32_t world, int mode) {
  if (!rd || rd->built || !world || rank >= world || (mode != ORCGPU_SHARD_STRIPES && mode != ORCGPU_SHARD_COLUMNS)) return ORCGPU_INVALID_ARGUMENT;
  rd->shard_rank = rank;
  rd->shard_world = world;
  rd->shard_mode = mode;
  return ORCGPU_OK;
}
int orcgpu_shard_columns(const double* weights, uint32_t n, uint32_t world, uint32_t* rank_of) {
  if (!world || (n && (!weights || !rank_of))) return ORCGPU_INVALID_ARGUMENT;
  orcgpu_host::lpt_deal(weights, n, world, rank_of);
  return ORCGPU_OK;
}
double orcgpu_reader_column_weight(const orcgpu_reader* rd, uint32_t root) {
  if (!rd || rd->md.types.empty() || root >= rd->md.types[0].subtypes.size()) return 0.0;
  return orcgpu_host::type_weight(rd->md.types, rd->md.types[0].subtypes[root]);
}
int orcgpu_reader_set_byte_range(orcgpu_reader* rd, uint64_t start, uint64_t end) {
  if (!rd || rd->built) return ORCGPU_INVALID_ARGUMENT;
  rd->has_range = true;
  rd->range_start = start;
  rd->range_end = end;
  return ORCGPU_OK;
}
int orcgpu_reader_set_timestamp_precision(orcgpu_reader* rd, int arrow_target) {
  if (!rd || rd->built || arrow_target < ORCGPU_ARROW_TIMESTAMP_S || arrow_target > ORCGPU_ARROW_TIMESTAMP_NS) return ORCGPU_INVALID_ARGUMENT;
  rd->ts_arrow_target = arrow_target;
  return ORCGPU_OK;
}
int orcgpu_reader_set_row_selection(orcgpu_reader* rd, const orcgpu_row_selector* selectors, uint32_t n) {
  if (!rd || rd->built || (n && !selectors)) return ORCGPU_INVALID_ARGUMENT;
  rd->selection = sel_normalise(selectors, n);
  rd->has_selection = true;
  return ORCGPU_OK;
}
uint64_t orcgpu_reader_total_rows(const orcgpu_reader* rd) { return rd ? rd->md.number_of_rows : 0; }
uint32_t orcgpu_reader_stripe_count(const orcgpu_reader* rd) { return rd ? (uint32_t)rd->md.stripes.size() : 0; }
uint32_t orcgpu_reader_column_count(orcgpu_reader* rd) {
  if (!rd) return 0;
  if (orcgpu_host::reader_build(rd)) return 0;
  return (uint32_t)rd->col_names.size();
}
const char* orcgpu_reader_column_name(orcgpu_reader* rd, uint32_t i) {
  if (!rd || orcgpu_host::reader_build(rd) || i >= rd->col_names.size()) return nullptr;
  return rd->col_names[i].c_str();
}

int orcgpu_index_entry(const orcgpu_column* column, int has_present, int compressed, const uint64_t* positions, uint32_t n_positions,
                       int32_t kind, orcgpu_stream_entry* out) {
  if (!column || (n_positions && !positions) || !out) return ORCGPU_INVALID_ARGUMENT;
  orcgpu_host::EntrySplit sp;
  if (!orcgpu_host::split_index_entry(column->orc_type, column->encoding, has_present != 0, compressed != 0, positions, n_positions, sp)) return ORCGPU_OUT_OF_SPEC;
  if (kind == ORCGPU_S_PRESENT && has_present) *out = sp.present;
  else if (kind == ORCGPU_S_DATA && sp.has_data) *out = sp.data;
  else if (sp.has_second && kind == sp.second_kind) *out = sp.second;
  else return ORCGPU_INVALID_ARGUMENT;  // a stream without positions (dictionaries), or one the column does not have
  return ORCGPU_OK;
}

// ArrowReader::next (arrow_reader.rs:333-346): 0 = a batch was exported, ORCGPU_END_OF_FILE = no more batches, else an error code
// (the end has a code of its own: the status of a failing batch may be any OrcError, ORCGPU_IO_ERROR = 1 included)
// (out_array: the host path; out_device: the device path -- the reader is in one mode or the other, and the wrong call changes nothing)
static int reader_next_stripe(orcgpu_reader* rd);
// The row filter's program, compiled at the first call that reads; a refusal is final and ends the reader
static int reader_ready_filter(orcgpu_reader* rd) {
  if (rd->filter_failed) return ORCGPU_END_OF_FILE;  // (the filter was refused by the call before: the iterator has ended)
  if (rd->has_filter && !rd->filter_ready) {
    const int rc = orcgpu_host::reader_compile_filter(rd);
    if (rc) {
      rd->filter_failed = true;
      rd->next_stripe = rd->stripe_order.size();
      return rc;
    }
    rd->filter_ready = true;
  }
  return ORCGPU_OK;
}
static int reader_next(orcgpu_reader* rd, struct ArrowArray* out_array, struct ArrowDeviceArray* out_device, struct ArrowSchema* out_schema) {
  if (!rd || (!out_array && !out_device) || !out_schema) return ORCGPU_INVALID_ARGUMENT;
  if (rd->has_aggs) {
    set_err(rd->ctx, "this reader aggregates (orcgpu_reader_set_aggregates): call orcgpu_reader_aggregate, it hands out no batches");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (rd->device_output != (out_device != nullptr)) {
    set_err(rd->ctx, rd->device_output ? "this reader hands out device batches (orcgpu_reader_set_device_output): call orcgpu_reader_next_batch_device"
                                       : "orcgpu_reader_next_batch_device needs orcgpu_reader_set_device_output before the first batch");
    return ORCGPU_INVALID_ARGUMENT;
  }
  int rc = orcgpu_host::reader_build(rd);
  if (rc) return rc;
  if (rd->device_output && !rd->stripe_order.empty() && !rd->device_checked) {
    // flat schemas only: a nested root column is refused before anything of the file is read (a file without stripes has no first
    // batch to fail: it ends as on the host path).  Checked once; a refusal is final
    rd->device_checked = true;
    for (size_t k = 0, root = 0; k < rd->col_ids.size() && !rd->device_refused; k++) {
      if (rd->col_parent[k]) continue;
      const std::string& name = rd->col_names[root++];
      const int kind = rd->md.types[rd->col_ids[k]].kind;
      if (kind == ORCGPU_T_STRUCT || kind == ORCGPU_T_LIST || kind == ORCGPU_T_MAP || kind == ORCGPU_T_UNION) {
        rd->device_refused = true;
        rd->device_refused_name = name;
        rd->device_refused_kind = kind == ORCGPU_T_STRUCT ? "Struct" : (kind == ORCGPU_T_LIST ? "List" : (kind == ORCGPU_T_MAP ? "Map" : "Union"));
      }
    }
  }
  if (rd->device_refused) return refuse_nested(rd->ctx, rd->device_refused_name, rd->device_refused_kind);
  rc = reader_ready_filter(rd);
  if (rc) return rc;
  for (;;) {
    if (rd->current) {
      uint32_t eb = 0, ec = 0;
      int st = orcgpu_result_status(rd->current, &eb, &ec);
      if (st && rd->next_batch >= eb) {
        orcgpu_host::reader_stop_worker(rd);  // the reference's iterator ends after an error
        set_err(rd->ctx, "stripe decode failed in batch %u, column %u", eb, ec);
        orcgpu_result_free(rd->current);
        rd->current = nullptr;
        rd->next_stripe = rd->stripe_order.size();
        return st;
      }
      if (rd->next_batch < orcgpu_result_batches(rd->current)) {
        // (the exported schema owns copies of the column names: it may outlive the reader)
        if (out_device) return export_batch_device_named(rd->ctx, rd->current, rd->next_batch++, out_device, out_schema, &rd->col_names);
        rc = export_batch_named(rd->ctx, rd->current, rd->next_batch++, out_array, out_schema, &rd->col_names);
        if (!rd->current_counted) {  // (the stripe's copy back has been started by now, by the worker or by this export)
          rd->d2h_bytes += rd->current->d2h_bytes;
          rd->current_counted = true;
        }
        return rc;
      }
    }
    rc = reader_next_stripe(rd);  // (ORCGPU_END_OF_FILE: every stripe has been handed out)
    if (rc) return rc;
  }
}

// The next decoded stripe becomes rd->current; the one before goes back, for a later stripe to be decoded into its buffers (by the
// worker, or by this thread when there is none).  ORCGPU_END_OF_FILE: there is no further stripe.
static int reader_next_stripe(orcgpu_reader* rd) {
  if (rd->current) {
    {
      std::lock_guard<std::mutex> g(rd->m);
      orcgpu_host::reader_give_spare(rd, rd->current);
    }
    rd->current = nullptr;
  }
  if (!rd->prefetch) return orcgpu_host::reader_advance_stripe(rd);
  if (!rd->worker_started) {
    if (rd->stripe_order.empty()) return ORCGPU_END_OF_FILE;
    // the stripe footers are decompressed by the GPU kernels on the decode stream: all of them now, before the two threads
    // share the context (from here on the stager only copies, the decoder only decodes)
    orcgpu_host::reader_read_metadata_ahead(rd);
    // (a footer that cannot be read is reported when its stripe's turn comes)
    // (a footer that cannot be read: the stripes before it are still handed out, the error arrives in its place)
    rd->worker_started = true;
    rd->stager = std::thread(orcgpu_host::reader_stager, rd);
    rd->decoder = std::thread(orcgpu_host::reader_decoder, rd);
  }
  orcgpu_reader::Ready item;
  {
    std::unique_lock<std::mutex> g(rd->m);
    rd->cv_ready.wait(g, [rd] { return !rd->ready.empty() || rd->worker_done; });
    if (rd->ready.empty()) return ORCGPU_END_OF_FILE;  // every stripe has been handed out
    item = std::move(rd->ready.front());
    rd->ready.pop_front();
  }
  rd->cv_room.notify_all();
  if (item.rc) {
    orcgpu_host::reader_stop_worker(rd);
    rd->ctx->err = item.err;
    return item.rc;
  }
  rd->current = item.res;
  rd->next_batch = 0;
  rd->current_counted = false;
  return ORCGPU_OK;
}

int orcgpu_reader_next_batch(orcgpu_reader* rd, struct ArrowArray* out_array, struct ArrowSchema* out_schema) {
  if (!out_array) return ORCGPU_INVALID_ARGUMENT;
  return reader_next(rd, out_array, nullptr, out_schema);
}
int orcgpu_reader_next_batch_device(orcgpu_reader* rd, struct ArrowDeviceArray* out_array, struct ArrowSchema* out_schema) {
  if (!out_array) return ORCGPU_INVALID_ARGUMENT;
  return reader_next(rd, nullptr, out_array, out_schema);
}
int orcgpu_reader_set_aggregates(orcgpu_reader* rd, const orcgpu_agg_spec* specs, uint32_t n_specs) {
  if (!rd || rd->built || !specs || !n_specs || n_specs > ORCGPU_AGG_MAX) return ORCGPU_INVALID_ARGUMENT;
  rd->agg_specs.assign(n_specs, {});
  for (uint32_t k = 0; k < n_specs; k++) {
    orcgpu_reader::AggSpec& s = rd->agg_specs[k];
    s.op = specs[k].op;
    s.has_column = specs[k].column != nullptr;
    s.has_column2 = specs[k].column2 != nullptr;
    if (s.has_column) s.column = specs[k].column;
    if (s.has_column2) s.column2 = specs[k].column2;
  }
  rd->has_aggs = true;
  return ORCGPU_OK;
}
// Drains the reader: every stripe's records, merged in stripe order, then the values
int orcgpu_reader_aggregate(orcgpu_reader* rd, orcgpu_agg_value* out) {
  if (!rd || !out) return ORCGPU_INVALID_ARGUMENT;
  if (!rd->has_aggs) {
    set_err(rd->ctx, "orcgpu_reader_aggregate needs orcgpu_reader_set_aggregates before the first call");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (rd->aggs_done) return ORCGPU_END_OF_FILE;
  int rc = orcgpu_host::reader_build(rd);
  if (rc) return rc;
  rd->aggs_done = true;  // (whatever comes of it: an error ends the reader as it ends an iterator)
  rc = orcgpu_host::reader_compile_aggs(rd);
  if (!rc) rc = reader_ready_filter(rd);
  if (rc) {
    rd->next_stripe = rd->stripe_order.size();
    return rc;
  }
  const std::vector<AggInsn>& insns = rd->agg_plan.insns;
  std::vector<AggPartial> total(insns.size(), AggPartial{});
  while (!(rc = reader_next_stripe(rd))) {
    const std::vector<AggPartial>& part = rd->current->agg_records;
    if (part.size() != insns.size() + 1) {
      set_err(rd->ctx, "aggregate: a stripe came without its records");
      rc = ORCGPU_UNEXPECTED;
      break;
    }
    for (size_t k = 0; k < insns.size(); k++) orcgpu_host::agg_merge(insns[k], total[k], part[k]);
  }
  if (rc != ORCGPU_END_OF_FILE) {
    orcgpu_host::reader_stop_worker(rd);
    rd->next_stripe = rd->stripe_order.size();
    return rc;
  }
  for (size_t k = 0; k < insns.size(); k++) orcgpu_host::agg_finish(insns[k], total[k], &out[k]);
  return ORCGPU_OK;
}
int orcgpu_reader_set_device_output(orcgpu_reader* rd, int on) {
  if (!rd || rd->built) return ORCGPU_INVALID_ARGUMENT;
  rd->device_output = on != 0;
  if (rd->device_output && !rd->home) rd->home = std::make_shared<orcgpu_hold::Home>();
  return ORCGPU_OK;
}
int orcgpu_reader_reads_ahead(orcgpu_reader* rd) {
  if (!rd) return 0;
  std::lock_guard<std::mutex> g(rd->m);
  return rd->worker_started && !rd->worker_done && !rd->stop ? 1 : 0;
}
int orcgpu_reader_d2h_bytes(const orcgpu_reader* rd, uint64_t* bytes) {
  if (!rd || !bytes) return ORCGPU_INVALID_ARGUMENT;
  *bytes = rd->d2h_bytes;
  return ORCGPU_OK;
}

}  // extern "C"
