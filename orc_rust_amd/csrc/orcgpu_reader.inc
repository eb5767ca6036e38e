// orcgpu_reader.inc -- host-side mirror of the reference's reader API for this path (C++ above the
// C ABI, because the reference is compiled code and there is no Rust toolchain in the image):
//
//   ChunkReader                      src/reader/mod.rs:27-76      (len / get_bytes; File and Bytes)
//   Stripe::new / StreamMap          src/stripe.rs:127-182, :311-336
//   ProjectionMask::{all,named_roots} src/projection.rs:30-69
//   ArrowReaderBuilder               src/arrow_reader.rs:39-231   (try_new, with_batch_size,
//                                    with_projection, with_file_byte_range, with_timestamp_precision, build)
//   ArrowReader / Cursor             src/arrow_reader.rs:233-392  (next, total_row_count)
//
// This file: the reader handle, the staging of a stripe's streams, the serial path and the two read-ahead threads.  Around it:
//   orcgpu_reader_meta.inc   file tail, stripe footers and row indexes, expanded by the GPU block decompressors
//   orcgpu_reader_plan.inc   what is read of the file and of each stripe, and how staged pieces are grouped: plain arithmetic,
//                            free of the device and of this handle (tests/hostcheck/reader_plan_check.cpp)
//   orcgpu_reader_api.inc    the C ABI
// Flat root columns are decoded, and Struct / List / Map / Union columns of them to any depth the decoder takes; a type kind
// beyond those is UnsupportedTypeVariant.
#include "orcgpu_reader_meta.inc"
#include "orcgpu_reader_plan.inc"
static_assert(orcgpu_host::kMetaMaxTypeDepth == kMaxTypeDepth, "the projection walk follows a type tree as deep as the decoder takes");

// ---- ArrowReaderBuilder + ArrowReader behind one handle -----------------------------------------------------
struct orcgpu_reader {
  orcgpu_ctx* ctx = nullptr;
  std::unique_ptr<orcgpu_host::ChunkReader> reader;
  orcgpu_host::FileMetadata md;
  // ---- the builder's options (ArrowReaderBuilder; orcgpu_reader_set_*, until the reader is built) ----
  uint32_t batch_size = 8192;                 // DEFAULT_BATCH_SIZE (arrow_reader.rs:37)
  orcgpu_host::ProjectionOptions opt;         // projection, with_schema, shard, dictionary columns, timestamp precision
  bool has_range = false;
  uint64_t range_start = 0, range_end = 0;    // with_file_byte_range
  bool has_selection = false;                 // with_row_selection
  std::vector<RowSel> selection;              // what is left of it for the stripes to come
  bool has_predicate = false;                 // with_predicate
  std::vector<orcgpu_host::PredNode> predicate;
  bool prune = true;                          // row groups under a row selection (orcgpu_reader_set_row_group_pruning)
  uint32_t prefetch = 2;                      // decoded stripes the reader may be ahead of the caller
  bool has_filter = false;                    // row filter (orcgpu_reader_set_row_filter): the nodes as given
  std::vector<orcgpu_host::PredNode> filter_nodes;
  // aggregates (orcgpu_reader_set_aggregates): the specs as given (their strings copied)
  bool has_aggs = false;
  struct AggSpec {
    uint32_t op = 0;
    bool has_column = false, has_column2 = false;
    std::string column, column2;
    // the spec's expression (orcgpu_reader_set_aggregate_exprs), nodes in pre-order with their names and literal bytes copied
    struct ExprNode {
      orcgpu_agg_expr_node n{};
      bool has_column = false, has_s = false;
      std::string column, s;
    };
    std::vector<ExprNode> expr;
    // the spec's condition (orcgpu_reader_set_aggregate_filters): its nodes with their names and literal bytes copied; none: empty
    std::vector<orcgpu_host::PredNode> filter;
  };
  std::vector<AggSpec> agg_specs;
  // GROUP BY (orcgpu_reader_set_group_by): the key columns as given
  bool has_group = false;
  std::vector<std::string> group_keys;
  uint32_t group_max = ORCGPU_GROUP_MAX, group_max_total = ORCGPU_GROUP_MAX_TOTAL;  // its limits (orcgpu_reader_set_group_limits)
  // ORDER BY ... LIMIT k (orcgpu_reader_set_top_k): the keys as given (their names copied)
  bool has_top_k = false;
  struct SortKey {
    std::string column;
    uint32_t descending = 0, nulls_first = 0;
  };
  std::vector<SortKey> top_k_keys;
  uint32_t top_k_k = 0;
  // device output (orcgpu_reader_set_device_output): the batches are views of the results' HBM, handed out by
  // orcgpu_reader_next_batch_device; no copy back is started.  A result the caller is done with goes to `home` instead of `spare`
  // -- at once, or when the last exported batch or tensor that views it is released (device_hold.h)
  bool device_output = false;
  std::shared_ptr<orcgpu_hold::Home> home;
  // ---- the projection (reader_build) ----
  bool built = false;
  std::vector<size_t> stripe_order;           // Cursor::get_stripe_metadatas
  orcgpu_host::Projection proj;               // every projected column: roots, and below a nested column its children (pre-order)
  // ---- iteration state (ArrowReader) ----
  size_t next_stripe = 0;
  orcgpu_result* current = nullptr;
  uint32_t next_batch = 0;
  std::vector<orcgpu_host::StripeFooter> footers;  // of the stripes of stripe_order, read (through the GPU decompressors) before the threads start
  bool footers_read = false;                  // ... and then: why the reading stopped early, if it did
  int footers_rc = 0;
  std::string footers_err;
  std::atomic<uint64_t> groups_read{0}, groups_total{0};
  std::deque<orcgpu_result*> serial_q;        // prefetch = 0: pieces of the current stripe decoded and not handed out yet
  // the row filter's program, from the first next_batch on
  bool filter_ready = false, filter_failed = false;
  orcgpu_host::FilterPlan filter_plan;
  std::atomic<uint64_t> filter_seen{0}, filter_kept{0}, filter_overflow{0};
  // the aggregates' instructions, from orcgpu_reader_aggregate on; every decoded stripe is aggregated where the filter and the
  // copy back would stand
  bool aggs_done = false;
  orcgpu_host::AggPlan agg_plan;
  orcgpu_host::GroupPlan group_plan;
  // the top-k's keys against the projected root columns, from the first next_batch on; the key records of the rows handed out so
  // far, stripe by stripe in hand-out order (orcgpu_reader_top_k_order merges them once the file has ended)
  bool top_k_ready = false, top_k_eof = false;
  orcgpu_host::TopKPlan top_k_plan;
  std::vector<orcgpu_host::TopKStripe> top_k_stripes;
  // orcgpu_reader_collect_keys: every decoded stripe gives the kept rows' keys of one column to a key set, where the aggregation
  // would stand; like it, the reader then hands out no batch and copies nothing back
  bool has_collect = false;
  struct orcgpu_key_set* collect_set = nullptr;
  uint32_t collect_col = 0;
  // orcgpu_reader_collect_map: the same drain into a key map (collect_set is its set then), with the value columns beside the key
  struct orcgpu_key_map* collect_map = nullptr;
  std::vector<uint32_t> collect_values;
  // lookup columns (orcgpu_reader_set_lookup_columns): the columns as given -- names copied, of each map what a probe needs and a
  // share of its memory, so that the handle may be freed --; from reader_build on their plan, which every staged stripe carries
  // into its decode call, and their names behind the roots' and in front of the computed columns' in proj.names
  bool has_lookup = false;
  struct LookupSpecCopy {
    std::string name, key_column;
    std::shared_ptr<orcgpu_host::LookupMapRef> map;
    uint32_t value = 0;
  };
  std::vector<LookupSpecCopy> lookup_specs;
  std::shared_ptr<orcgpu_host::LookupPlan> lookup_plan;
  // computed columns (orcgpu_reader_set_computed_columns): the columns as given (their names and nodes copied); from reader_build
  // on their plan, which every staged stripe carries into its decode call, and their names behind the roots' in proj.names
  bool has_computed = false;
  struct ComputedSpec {
    std::string name;
    std::vector<AggSpec::ExprNode> expr;
  };
  std::vector<ComputedSpec> computed_specs;
  std::shared_ptr<orcgpu_host::ComputedPlan> computed_plan;
  int computed_rc = 0;                        // their refusal, final: every later call that builds the reader gets it again
  std::string computed_err;
  std::atomic<uint64_t> computed_overflow{0}; // rows decoded so far whose computed value overflowed (orcgpu_reader_computed_overflow_rows)
  uint64_t d2h_bytes = 0;                     // column-buffer bytes copied to the host so far (orcgpu_reader_d2h_bytes)
  bool current_counted = false;               // ... those of `current` are in it
  bool device_checked = false, device_refused = false;  // the projection has been looked at for nested columns; it has one
  std::string device_refused_name;
  const char* device_refused_kind = "";
  // ---- read-ahead (the analogue of async_arrow_reader.rs:165-280, whose state machine fetches the next stripe while the
  // caller consumes the batches of the current one).  Two threads of the reader own its GPU calls: the STAGER reads the
  // streams of the stripes to come from the file and stages them in HBM (copy stream); the DECODER takes the stripes staged
  // so far -- several per call when it is the slower of the two: short stripes then share their kernel launches --, decodes
  // them, starts their copies back to the host (device-to-host stream) and queues them.  The caller's thread only waits for
  // a copy and hands out views of the pinned host buffers.  In steady state reading + staging (k + 1), decoding (k) and the
  // copy back of (k - 1) overlap.  prefetch = 0: everything in the caller's thread, one stripe after the other. ----
  struct Ready {
    orcgpu_result* res = nullptr;
    int rc = 0;
    std::string err;
  };
  std::thread stager, decoder;
  std::mutex m;
  std::condition_variable cv_room, cv_ready, cv_staged, cv_staged_room;
  std::deque<orcgpu_staged*> staged_q;        // staged, not yet decoded (stager -> decoder)
  int stager_rc = 0;                          // why the stager stopped early (0: it did not)
  std::string stager_err;
  std::deque<Ready> ready;                    // decoded, copy back under way (decoder -> caller)
  std::vector<orcgpu_result*> spare;          // results the caller is done with: their buffers are decoded into again
  bool worker_started = false, stager_done = false, worker_done = false, stop = false;
};

namespace orcgpu_host {

// ctx->err behind its lock (set_err writes it under the same one): the workers' errors travel through the reader as strings
std::string ctx_err_text(orcgpu_ctx* c) {
  std::lock_guard<std::mutex> g(c->err_m);
  return c->err;
}
void ctx_err_put(orcgpu_ctx* c, const std::string& text) {
  std::lock_guard<std::mutex> g(c->err_m);
  c->err = text;
}

int reader_compile_computed(orcgpu_reader* rd);
int reader_compile_lookup(orcgpu_reader* rd);
int reader_build(orcgpu_reader* rd) {
  if (rd->built && rd->computed_rc) set_err(rd->ctx, "%s", rd->computed_err.c_str());
  if (rd->built) return rd->computed_rc;
  rd->built = true;
  rd->stripe_order.clear();
  for (size_t i = 0; i < rd->md.stripes.size(); i++) {
    uint64_t off = rd->md.stripes[i].offset;
    if (!rd->has_range || (off >= rd->range_start && off < rd->range_end)) rd->stripe_order.push_back(i);
  }
  MetaErr e;
  const int rc = build_projection(rd->md, rd->opt, rd->proj, e);
  if (rc && e.msg[0]) set_err(rd->ctx, "%s", e.msg);
  if (!rc && (rd->has_computed || rd->has_lookup)) {  // (a refusal ends the reader: nothing of the file is read)
    // the lookup columns first: their names stand in front of the computed columns'.  (computed_rc / _err keep either's refusal)
    rd->computed_rc = rd->has_lookup ? reader_compile_lookup(rd) : ORCGPU_OK;
    if (!rd->computed_rc && rd->has_computed) rd->computed_rc = reader_compile_computed(rd);
    if (rd->computed_rc) {
      rd->computed_err = ctx_err_text(rd->ctx);
      rd->next_stripe = rd->stripe_order.size();
    }
    return rd->computed_rc;
  }
  return rc;
}

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
  std::vector<orcgpu_column> cols = stripe_columns(rd->md, sf, rd->proj, rd->opt);
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
  const int rc = orcgpu_stage_stripe(ctx, &d, staged_out);  // (the caller's buffers may go as soon as it returns)
  if (!rc && rd->lookup_plan) (*staged_out)->lookup = rd->lookup_plan;        // (the decode call appends the lookup columns ...)
  if (!rc && rd->computed_plan) (*staged_out)->computed = rd->computed_plan;  // (... and the computed columns behind them)
  return rc;
}

// The footer of stripe number `at` of the reader's stripes: the one read ahead, or read now into `local`
int reader_stripe_footer(orcgpu_reader* rd, size_t at, const StripeInfo& si, StripeFooter& local, StripeFooter** sf) {
  *sf = at < rd->footers.size() ? &rd->footers[at] : &local;
  if (at < rd->footers.size()) return ORCGPU_OK;
  if (rd->footers_read) {  // (read-ahead: this footer is the one that could not be read)
    set_err(rd->ctx, "%s", rd->footers_err.c_str());
    return rd->footers_rc ? rd->footers_rc : ORCGPU_UNEXPECTED;
  }
  return read_stripe_footer(rd->ctx, *rd->reader, rd->md, si, local);
}

// arrow_reader.rs:258-293: the predicate against the stripe's row indexes -> the row groups to keep.  false: the evaluation failed
bool reader_predicate_groups(orcgpu_reader* rd, StripeFooter& sf, uint64_t n_rows, std::vector<uint8_t>& keep) {
  if (!sf.index_read && read_stripe_index(rd->ctx, *rd->reader, rd->md, sf, rd->proj.ids(), true)) sf.index.clear();
  std::vector<std::string> names;
  std::vector<ColumnGroups> cols;
  for (size_t k : rd->proj.roots())
    for (auto& ci : sf.index)
      if (ci.column == rd->proj.cols[k].id && ci.has_groups) {
        names.push_back(rd->proj.names[rd->proj.cols[k].root]);
        cols.push_back(ci.groups);
      }
  const uint64_t stride = rd->md.row_index_stride;
  const uint64_t ng = stride ? (n_rows + stride - 1) / stride : 0;
  std::vector<std::string> computed;  // (the statistics know nothing of them: a leaf on one keeps every row group)
  if (rd->lookup_plan)
    for (const LookupColumn& c : rd->lookup_plan->cols) computed.push_back(c.name);
  if (rd->computed_plan)
    for (const ComputedColumn& c : rd->computed_plan->cols) computed.push_back(c.name);
  return predicate_row_groups(rd->predicate, names, cols, (size_t)ng, keep, computed.empty() ? nullptr : &computed);
}

// The next stripe of the file -> staged rows: the whole stripe, or -- under a row selection, when its ROW_INDEX streams allow
// it -- one staged piece per run of consecutive row groups that hold selected rows (none: the stripe is not read at all).
int reader_stage_next(orcgpu_reader* rd, std::vector<orcgpu_staged*>& out) {
  const size_t at = rd->next_stripe++;
  const StripeInfo& si = rd->md.stripes[rd->stripe_order[at]];
  // is this stripe this rank's
  if (!stripe_is_mine(rd->opt, at)) {
    // another rank's stripe: it still takes its share of the row selection (arrow_reader.rs:296-308), nothing of it is read
    if (rd->has_selection && sel_row_count(rd->selection) > 0) (void)sel_split_off(rd->selection, si.number_of_rows);
    return ORCGPU_OK;
  }
  // the footer for this stripe
  StripeFooter local, *sf = nullptr;
  int rc = reader_stripe_footer(rd, at, si, local, &sf);
  if (rc) return rc;
  // the stripe's selection: the predicate's row groups, and its share of the row selection (arrow_reader.rs:296-308; with no rows
  // left in it, stripes are read whole)
  StripeAsk ask;
  ask.n_rows = si.number_of_rows;
  ask.stride = rd->md.row_index_stride;
  ask.batch_size = rd->batch_size;
  ask.prune = rd->prune;
  ask.has_filter = rd->has_filter;
  ask.has_predicate = rd->has_predicate;
  std::vector<uint8_t> keep;
  if (rd->has_predicate) ask.predicate_ok = reader_predicate_groups(rd, *sf, ask.n_rows, keep);
  ask.keep = &keep;
  std::vector<RowSel> share;
  const bool has_share = rd->has_selection && sel_row_count(rd->selection) > 0;
  if (has_share) share = sel_split_off(rd->selection, ask.n_rows);
  // plan (an index that cannot be read: the stripe is decoded whole)
  StagePlan plan = plan_stripe(rd->md, *sf, rd->proj, *rd->reader, ask, has_share ? &share : nullptr, [&] {
    if (read_stripe_index(rd->ctx, *rd->reader, rd->md, *sf, rd->proj.ids(), false)) sf->index.clear();
  });
  rd->groups_total += plan.groups_total;
  // stage each planned piece
  for (StagePiece& piece : plan.stages) {
    orcgpu_staged* st = nullptr;
    rc = reader_stage_rows(rd, *sf, piece.pieces, piece.n_rows, &st);
    if (rc) return rc;
    st->has_sel = piece.has_sel;
    st->piece = piece.is_piece;
    st->sel = std::move(piece.sel);
    rd->groups_read += piece.groups;
    out.push_back(st);
  }
  return ORCGPU_OK;
}

// Every stripe footer of the file -- and, under a predicate or a row selection, the row indexes the stripes will be asked for --
// read now, by one call of the GPU decompressors each (rather than one or two calls per stripe as their turns come).
void reader_read_metadata_ahead(orcgpu_reader* rd) {
  auto owned = [rd](size_t at) { return stripe_is_mine(rd->opt, at); };
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
  if (n_read < infos.size()) rd->footers_err = ctx_err_text(rd->ctx);
  rd->footers.assign(n_upto, StripeFooter{});
  for (size_t k = 0; k < n_read; k++) rd->footers[at_of[k]] = std::move(got[k]);
  std::vector<StripeFooter*> want;
  const std::vector<uint32_t> col_ids = rd->proj.ids();
  if (rd->has_predicate) {
    // ... and so are the row indexes (statistics, Bloom filters, positions) of every stripe, for the predicate
    for (size_t k = 0; k < n_upto; k++)
      if (owned(k)) want.push_back(&rd->footers[k]);
    read_stripe_indexes(rd->ctx, *rd->reader, rd->md, want, col_ids, true);
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
    read_stripe_indexes(rd->ctx, *rd->reader, rd->md, want, col_ids, false);
  }
  rd->footers_read = true;
}

// The row filter on one decoded (and selected) stripe.  A stripe whose decode failed is left as it is: its error arrives with
// its failing batch.
int reader_filter_result(orcgpu_reader* rd, orcgpu_result* res) {
  if (res->status) return ORCGPU_OK;
  uint64_t seen = 0, kept = 0, overflow = 0;
  const int rc = result_filter_plan(rd->ctx, res, rd->filter_plan, &seen, &kept, nullptr, 0, &overflow);
  rd->filter_seen += seen;
  rd->filter_kept += kept;
  rd->filter_overflow += overflow;
  return rc;
}

// The filter's nodes against the projected root columns -> its program, once, at the first next_batch
int reader_compile_filter(orcgpu_reader* rd) {
  std::vector<const char*> names;
  std::vector<int32_t> kinds, params;
  for (size_t k : rd->proj.roots()) {
    // (a column below a Struct / List / Map / Union is no root: its root is refused by its kind)
    const ProjCol& pc = rd->proj.cols[k];
    const OrcType& t = rd->md.types[pc.id];
    names.push_back(rd->proj.names[pc.root].c_str());
    kinds.push_back(t.kind);
    // what a Decimal128 / TimestampNs literal is brought to: the column's scale (with_schema takes no other), the unit it is decoded to
    orcgpu_column c{};
    c.arrow_target = rd->opt.has_schema ? pc.target : rd->opt.ts_arrow_target;
    params.push_back(t.kind == ORCGPU_T_DECIMAL ? (int32_t)t.scale : ts_unit_of(c));
  }
  if (rd->lookup_plan)  // the lookup columns behind the roots: Long, Decimal(p, s) or Double
    for (const LookupColumn& c : rd->lookup_plan->cols) {
      names.push_back(c.name.c_str());
      kinds.push_back(lookup_orc_type(c.v));
      params.push_back(c.v.kind == KMV_DEC128 ? (int32_t)c.v.scale : 3);
    }
  if (rd->computed_plan)  // the computed columns behind them: Long, Decimal(38, s) or Double
    for (const ComputedColumn& c : rd->computed_plan->cols) {
      names.push_back(c.name.c_str());
      kinds.push_back(computed_orc_type(c));
      params.push_back(c.cls == XCLASS_DEC ? c.scale : 3);
    }
  const std::vector<orcgpu_predicate_node> nodes = view_predicate(rd->filter_nodes);
  const KeySetRefs sets = ctx_key_set_refs(rd->ctx);  // (what a set leaf may name; the plan holds the memory of the ones it does)
  const int rc = filter_compile(nodes.data(), (uint32_t)nodes.size(), names.data(), kinds.data(), (uint32_t)names.size(), rd->filter_plan, params.data(), &sets);
  if (rc) set_err(rd->ctx, "%s", rd->filter_plan.err);
  if (rc) return rc;
  // a comparison on a dictionary-output column would have to be evaluated on the entries: refused, by name, before anything is read
  const std::vector<size_t> roots = rd->proj.roots();
  for (auto& in : rd->filter_plan.prog) {
    std::vector<uint32_t> read;  // the columns whose values the leaf reads: its own, or every one an expression leaf names
    if (in.op == FOP_CMP_EXPR) {
      std::vector<FilterExprRead> reads;
      filter_expr_reads(rd->filter_plan, in, reads);
      for (const FilterExprRead& x : reads)
        if (x.kind != kFilterExprAnyKind) read.push_back(x.col);
    } else if (fop_reads_values(in.op)) read.push_back(in.col);
    for (const uint32_t col : read) {
      if (col >= roots.size() || !rd->proj.cols[roots[col]].dict) continue;  // (past the roots: a computed column)
      set_err(rd->ctx, "row filter: column '%s' is read as a dictionary column (orcgpu_reader_set_dictionary_columns): a comparison on it is not supported", names[col]);
      return ORCGPU_UNSUPPORTED;
    }
  }
  return ORCGPU_OK;
}

// The reader's copies as the C arrays the plan compiler takes: specs and, parallel to them, exprs (whose nodes live in `nodes`)
struct ReaderAggView {
  std::vector<orcgpu_agg_spec> specs;
  std::vector<orcgpu_agg_expr> exprs;
  std::vector<std::vector<orcgpu_agg_expr_node>> nodes;
  std::vector<orcgpu_agg_filter> filters;  // parallel too: the specs' conditions, whose nodes live in `filter_nodes`
  std::vector<std::vector<orcgpu_predicate_node>> filter_nodes;
};
void reader_view_aggs(const orcgpu_reader* rd, ReaderAggView& v) {
  const size_t n = rd->agg_specs.size();
  v.specs.resize(n);
  v.exprs.assign(n, orcgpu_agg_expr{nullptr, 0});
  v.nodes.assign(n, {});
  v.filters.assign(n, orcgpu_agg_filter{nullptr, 0});
  v.filter_nodes.assign(n, {});
  for (size_t k = 0; k < n; k++) {
    const orcgpu_reader::AggSpec& s = rd->agg_specs[k];
    v.specs[k] = {s.op, s.has_column ? s.column.c_str() : nullptr, s.has_column2 ? s.column2.c_str() : nullptr};
    for (const auto& e : s.expr) {
      orcgpu_agg_expr_node x = e.n;
      x.column = e.has_column ? e.column.c_str() : nullptr;
      x.s = e.has_s ? e.s.data() : nullptr;
      v.nodes[k].push_back(x);
    }
    if (!v.nodes[k].empty()) v.exprs[k] = {v.nodes[k].data(), (uint32_t)v.nodes[k].size()};
    if (!s.filter.empty()) {
      v.filter_nodes[k] = view_predicate(s.filter);
      v.filters[k] = {v.filter_nodes[k].data(), (uint32_t)v.filter_nodes[k].size()};
    }
  }
}

// The aggregate list against the projected root columns as the file's metadata and the builder describe them -> its instructions,
// once, before anything is read: every refusal arrives here.  (What a stripe's decode made of the columns is checked again, per
// stripe, by the plan the kernels run: reader_aggregate_result.)
void reader_describe_file_roots(orcgpu_reader* rd, std::vector<const char*>& names, std::vector<AggCol>& cols) {
  for (size_t k : rd->proj.roots()) {
    const ProjCol& pc = rd->proj.cols[k];
    const OrcType& t = rd->md.types[pc.id];
    names.push_back(rd->proj.names[pc.root].c_str());
    orcgpu_column c{};
    c.arrow_target = rd->opt.has_schema ? pc.target : rd->opt.ts_arrow_target;
    AggCol a;
    a.d.orc_type = t.kind;
    a.d.ts_unit = ts_unit_of(c);
    a.d.is_bool = t.kind == ORCGPU_T_BOOLEAN;
    a.d.dict_out = pc.dict;
    a.d.is_string = !a.d.dict_out && (t.kind == ORCGPU_T_STRING || t.kind == ORCGPU_T_VARCHAR || t.kind == ORCGPU_T_CHAR || t.kind == ORCGPU_T_BINARY);
    const bool is_ts = t.kind == ORCGPU_T_TIMESTAMP || t.kind == ORCGPU_T_TIMESTAMP_INSTANT;
    a.d.width = t.kind == ORCGPU_T_BYTE ? 1 : t.kind == ORCGPU_T_SHORT ? 2 : (t.kind == ORCGPU_T_INT || t.kind == ORCGPU_T_FLOAT || t.kind == ORCGPU_T_DATE || a.d.dict_out) ? 4
                : (t.kind == ORCGPU_T_DECIMAL || (is_ts && a.d.ts_unit > 3)) ? 16 : (a.d.is_bool || a.d.is_string) ? 0 : 8;
    a.scale = t.scale;
    a.nested = is_nested_kind(t.kind);
    cols.push_back(a);
  }
}
// ... and behind them the computed columns, as what the decode call makes of them: Long, Decimal(38, s) or Double
void reader_describe_roots(orcgpu_reader* rd, std::vector<const char*>& names, std::vector<AggCol>& cols) {
  reader_describe_file_roots(rd, names, cols);
  if (rd->lookup_plan)
    for (const LookupColumn& c : rd->lookup_plan->cols) {
      names.push_back(c.name.c_str());
      AggCol a;
      a.d.orc_type = lookup_orc_type(c.v);
      a.d.width = key_map_value_width(c.v.kind);
      a.d.ts_unit = 3;
      a.d.has_present = true;
      a.scale = c.v.kind == KMV_DEC128 ? c.v.scale : 0;
      cols.push_back(a);
    }
  if (!rd->computed_plan) return;
  for (const ComputedColumn& c : rd->computed_plan->cols) {
    names.push_back(c.name.c_str());
    AggCol a;
    a.d.orc_type = computed_orc_type(c);
    a.d.width = computed_width(c);
    a.d.ts_unit = 3;
    a.d.has_present = true;
    a.scale = c.cls == XCLASS_DEC ? (uint32_t)c.scale : 0;
    cols.push_back(a);
  }
}
// The computed columns against the file's root columns and the projected ones, once, when the reader is built: every refusal
// arrives here.  Then their names stand behind the roots' wherever the reader's names are read (proj.names)
int reader_compile_computed(orcgpu_reader* rd) {
  std::vector<const char*> names;
  std::vector<AggCol> cols;
  reader_describe_file_roots(rd, names, cols);
  std::vector<AggExprCol> xcols;
  std::vector<uint8_t> nested;
  for (const AggCol& c : cols) {
    xcols.push_back(agg_expr_col(c));
    nested.push_back(c.nested ? 1 : 0);
  }
  std::vector<const char*> file_roots;
  if (!rd->md.types.empty())
    for (auto& n : rd->md.types[0].field_names) file_roots.push_back(n.c_str());
  std::vector<const char*> cnames;
  std::vector<orcgpu_agg_expr> exprs;
  std::vector<std::vector<orcgpu_agg_expr_node>> nodes(rd->computed_specs.size());
  for (size_t k = 0; k < rd->computed_specs.size(); k++) {
    const orcgpu_reader::ComputedSpec& s = rd->computed_specs[k];
    cnames.push_back(s.name.c_str());
    for (const auto& e : s.expr) {
      orcgpu_agg_expr_node x = e.n;
      x.column = e.has_column ? e.column.c_str() : nullptr;
      x.s = e.has_s ? e.s.data() : nullptr;
      nodes[k].push_back(x);
    }
    exprs.push_back({nodes[k].data(), (uint32_t)nodes[k].size()});
  }
  if (rd->lookup_plan)  // (an operand that is a lookup column is refused by name, before the compiler would call it unknown)
    for (size_t k = 0; k < nodes.size(); k++)
      for (const orcgpu_agg_expr_node& x : nodes[k]) {
        char err[320];
        if (x.op != ORCGPU_AGG_EXPR_COLUMN || !x.column) continue;
        if (const int rc = lookup_refuse_computed_operand(*rd->lookup_plan, cnames[k], x.column, err, sizeof(err))) {
          set_err(rd->ctx, "%s", err);
          return rc;
        }
      }
  auto plan = std::make_shared<ComputedPlan>();
  const int rc = computed_compile(cnames.data(), exprs.data(), (uint32_t)cnames.size(), file_roots.data(), (uint32_t)file_roots.size(), names.data(), xcols.data(),
                                  nested.data(), (uint32_t)names.size(), *plan);
  if (rc) {
    set_err(rd->ctx, "%s", plan->err);
    return rc;
  }
  for (const ComputedColumn& c : plan->cols) rd->proj.names.push_back(c.name);
  rd->computed_plan = std::move(plan);
  return ORCGPU_OK;
}
// The lookup columns against the file's root columns, the projected ones and the computed columns' names, once, when the reader is
// built and in front of the computed columns: every refusal arrives here.  Then their names stand behind the roots' in proj.names
int reader_compile_lookup(orcgpu_reader* rd) {
  std::vector<const char*> names;
  std::vector<AggCol> cols;
  reader_describe_file_roots(rd, names, cols);
  std::vector<LookupProjCol> pcols;
  for (const AggCol& c : cols) {
    LookupProjCol p;
    p.orc_type = c.d.orc_type;
    p.dict_read = c.d.dict_out;
    p.nested = c.nested;
    pcols.push_back(p);
  }
  std::vector<const char*> file_roots, computed;
  if (!rd->md.types.empty())
    for (auto& n : rd->md.types[0].field_names) file_roots.push_back(n.c_str());
  for (const orcgpu_reader::ComputedSpec& s : rd->computed_specs) computed.push_back(s.name.c_str());
  std::vector<LookupSpec> specs;
  for (const orcgpu_reader::LookupSpecCopy& s : rd->lookup_specs) {
    LookupSpec x;
    x.name = s.name.c_str();
    x.key_column = s.key_column.c_str();
    x.map = s.map.get();
    x.value = s.value;
    specs.push_back(x);
  }
  auto plan = std::make_shared<LookupPlan>();
  const int rc = lookup_compile(specs.data(), (uint32_t)specs.size(), file_roots.data(), (uint32_t)file_roots.size(), computed.data(), (uint32_t)computed.size(), names.data(),
                                pcols.data(), (uint32_t)names.size(), *plan);
  if (rc) {
    set_err(rd->ctx, "%s", plan->err);
    return rc;
  }
  for (const LookupColumn& c : plan->cols) rd->proj.names.push_back(c.name);
  rd->lookup_plan = std::move(plan);
  return ORCGPU_OK;
}
int reader_compile_aggs(orcgpu_reader* rd) {
  std::vector<const char*> names;
  std::vector<AggCol> cols;
  reader_describe_roots(rd, names, cols);
  ReaderAggView v;
  reader_view_aggs(rd, v);
  const KeySetRefs sets = ctx_key_set_refs(rd->ctx);
  const int rc = agg_compile(v.specs.data(), v.exprs.data(), v.filters.data(), (uint32_t)v.specs.size(), names.data(), cols.data(), (uint32_t)cols.size(), rd->agg_plan, &sets);
  if (rc) set_err(rd->ctx, "%s", rd->agg_plan.err);
  return rc;
}
// The reader's own strings as the C array the plan compilers and the calls take
static std::vector<const char*> reader_c_strings(const std::vector<std::string>& strings) {
  std::vector<const char*> out;
  for (auto& s : strings) out.push_back(s.c_str());
  return out;
}
// ... and the key list of a GROUP BY, against the same description
int reader_compile_group(orcgpu_reader* rd) {
  std::vector<const char*> names;
  const std::vector<const char*> keys = reader_c_strings(rd->group_keys);
  std::vector<AggCol> cols;
  reader_describe_roots(rd, names, cols);
  const int rc = group_compile(keys.data(), (uint32_t)keys.size(), names.data(), cols.data(), (uint32_t)cols.size(), rd->group_plan);
  rd->group_plan.max_groups = rd->group_max;  // (what the merge refuses the total against, and the flags check the stripe)
  rd->group_plan.max_total = rd->group_max_total;
  if (rc) set_err(rd->ctx, "%s", rd->group_plan.err);
  return rc;
}

// The aggregation of one decoded (and selected) stripe, where reader_filter_result and the copy back stand otherwise: its
// records stay with the result until orcgpu_reader_aggregate merges them, in stripe order.  A stripe whose decode failed ends the call.
int reader_aggregate_result(orcgpu_reader* rd, orcgpu_result* res) {
  if (res->status) {
    set_err(rd->ctx, "stripe decode failed in batch %u, column %u", res->err_batch, res->err_col);
    return res->status;
  }
  const std::vector<const char*> names = reader_c_strings(rd->proj.names), keys = reader_c_strings(rd->group_keys);
  if (names.size() != res->cols.size()) {  // (a flat projection: one result column per root column; anything else the plan has refused)
    set_err(rd->ctx, "aggregate: the result holds %zu columns for %zu projected root columns", res->cols.size(), names.size());
    return ORCGPU_UNSUPPORTED;
  }
  ReaderAggView v;
  reader_view_aggs(rd, v);
  AggPlan plan;
  if (const int rc = result_compile_aggs(rd->ctx, res, v.specs.data(), v.exprs.data(), v.filters.data(), (uint32_t)v.specs.size(), names.data(), plan)) return rc;
  for (size_t k = 0; k < plan.insns.size(); k++)
    if (plan.insns[k].kind != rd->agg_plan.insns[k].kind || plan.insns[k].scale != rd->agg_plan.insns[k].scale) {
      if (agg_is_expr(plan.insns[k].kind) || agg_is_expr(rd->agg_plan.insns[k].kind))  // (col is no column index then)
        set_err(rd->ctx, "aggregate: the columns of the expression of aggregate %zu are not decoded to the types it was planned for", k);
      else
        set_err(rd->ctx, "aggregate: column '%s' is not decoded to the type its aggregate was planned for", names[plan.insns[k].col]);
      return ORCGPU_MISMATCHED_SCHEMA;
    }
  GroupPlan gplan;
  if (rd->has_group) {  // the grouped reduction in the same place: the stripe's groups stay with the result
    if (const int rc = result_compile_group(rd->ctx, res, keys.data(), (uint32_t)keys.size(), names.data(), gplan)) return rc;
    gplan.max_groups = rd->group_max;  // (the limit picks the stripe's path: above ORCGPU_GROUP_MAX the wide one)
    gplan.max_total = rd->group_max_total;
    for (size_t k = 0; k < gplan.keys.size(); k++)
      if (gplan.keys[k].kind != rd->group_plan.keys[k].kind || gplan.keys[k].scale_or_unit != rd->group_plan.keys[k].scale_or_unit) {
        set_err(rd->ctx, "group by: key column '%s' is not decoded to the type its key was planned for", names[gplan.keys[k].col]);
        return ORCGPU_MISMATCHED_SCHEMA;
      }
  }
  GroupSet set;
  uint64_t kept = 0;
  const int rc = result_aggregate_call(rd->ctx, res, rd->has_filter ? &rd->filter_plan : nullptr, plan, rd->has_group ? &gplan : nullptr, set, &res->agg_seen, &kept,
                                       names.data(), (uint32_t)names.size());
  if (rc) return rc;
  if (rd->has_group) res->grp_keys = std::move(set.keys), res->grp_vals = std::move(set.vals);
  else res->agg_records = std::move(set.vals);
  rd->filter_seen += res->agg_seen;
  rd->filter_kept += kept;
  return ORCGPU_OK;
}

// The reader's sort keys as the C array the plan compiler takes
std::vector<orcgpu_sort_key> reader_view_sort_keys(const orcgpu_reader* rd) {
  std::vector<orcgpu_sort_key> keys;
  for (auto& k : rd->top_k_keys) keys.push_back({k.column.c_str(), k.descending, k.nulls_first});
  return keys;
}
// The sort keys against the projected root columns as the file's metadata and the builder describe them, once, before anything is
// read: every refusal arrives here.  (What a stripe's decode made of the columns is checked again per stripe: reader_top_k_result.)
int reader_compile_top_k(orcgpu_reader* rd) {
  std::vector<const char*> names;
  std::vector<AggCol> cols;
  reader_describe_roots(rd, names, cols);
  const std::vector<orcgpu_sort_key> keys = reader_view_sort_keys(rd);
  const int rc = top_k_compile(keys.data(), (uint32_t)keys.size(), rd->top_k_k, names.data(), cols.data(), (uint32_t)cols.size(), rd->top_k_plan);
  if (rc) set_err(rd->ctx, "%s", rd->top_k_plan.err);
  return rc;
}
// The top-k of one decoded (and selected) stripe, where reader_filter_result stands otherwise: behind the row filter's evaluation
// if there is one, its at most k best rows become the result's batches and their key records stay with the result until it is
// handed out.  A stripe whose decode failed is left as it is: its error arrives with its failing batch.
int reader_top_k_result(orcgpu_reader* rd, orcgpu_result* res) {
  res->top_k_records.clear();
  if (res->status) return ORCGPU_OK;
  std::vector<const char*> names;
  for (size_t k : rd->proj.roots()) names.push_back(rd->proj.names[rd->proj.cols[k].root].c_str());
  if (rd->lookup_plan)
    for (const LookupColumn& c : rd->lookup_plan->cols) names.push_back(c.name.c_str());
  if (rd->computed_plan)
    for (const ComputedColumn& c : rd->computed_plan->cols) names.push_back(c.name.c_str());
  if (names.size() != res->cols.size()) {
    set_err(rd->ctx, "top-k: the result holds %zu columns for %zu projected root columns", res->cols.size(), names.size());
    return ORCGPU_UNEXPECTED;
  }
  const std::vector<orcgpu_sort_key> keys = reader_view_sort_keys(rd);
  TopKPlan plan;
  if (const int rc = result_compile_top_k(rd->ctx, res, keys.data(), (uint32_t)keys.size(), rd->top_k_k, names.data(), plan)) return rc;
  if (plan.keys.len != rd->top_k_plan.keys.len || memcmp(&plan.keys, &rd->top_k_plan.keys, sizeof(plan.keys)) != 0) {
    set_err(rd->ctx, "top-k: the key columns are not decoded to the types the keys were planned for");
    return ORCGPU_MISMATCHED_SCHEMA;
  }
  uint64_t seen = 0, kept = 0;
  const int rc = result_top_k_plan(rd->ctx, res, rd->has_filter ? &rd->filter_plan : nullptr, plan, &seen, &kept, nullptr, &res->top_k_records, names.data(), (uint32_t)names.size());
  rd->filter_seen += seen;
  rd->filter_kept += kept;
  return rc;
}

int reader_collect_result(orcgpu_reader* rd, orcgpu_result* res);  // (orcgpu_key_set_call.inc)

// A result the caller is done with, to decode a later stripe into (rd->m is held by a reader that reads ahead)
orcgpu_result* reader_take_spare(orcgpu_reader* rd) {
  // (a result that comes home was viewed by batches and tensors whose consumers released them on the HOST: work they enqueued on
  // streams of their own may not have run yet, and nothing orders the decode stream behind it -- so decode_staged_once waits for
  // the device before it writes into a result that has been exported)
  if (rd->device_output && !rd->has_aggs && !rd->has_collect) return static_cast<orcgpu_result*>(orcgpu_hold::home_take(*rd->home));
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

// What follows the decode call for each of its results, on both paths: the field names, the stripe's share of the selection, the
// aggregation -- in place of the filter's compaction and of any copy back -- or the row filter (before the copy back is started:
// only the kept rows cross the link); the staged stripe is freed whatever came of it.  start_copy: the read-ahead path starts
// the copy back here, the serial host path copies back when the first batch is asked for
int reader_finish_decoded(orcgpu_reader* rd, orcgpu_staged* staged, orcgpu_result* res, bool start_copy, int rc) {
  if (!rc) {
    res->field_names.clear();
    for (auto& c : rd->proj.cols) res->field_names.push_back(c.field);
  }
  if (!rc) rd->computed_overflow += res->computed_overflow;  // (0 without computed columns)
  if (!rc && staged->has_sel) rc = result_select_batches(rd->ctx, res, staged->sel);
  if (!rc && rd->has_aggs) rc = reader_aggregate_result(rd, res);
  else if (!rc && rd->has_collect) rc = reader_collect_result(rd, res);
  else if (!rc && rd->has_top_k) rc = reader_top_k_result(rd, res);
  else if (!rc && rd->has_filter) rc = reader_filter_result(rd, res);
  orcgpu_staged_free(staged);
  if (!rc && !rd->has_aggs && !rd->has_collect) rc = reader_result_decoded(rd, res, start_copy);
  return rc;
}

// A decoded stripe becomes rd->current, its batches handed out from the first
void reader_make_current(orcgpu_reader* rd, orcgpu_result* res) {
  rd->current = res;
  rd->next_batch = 0;
  rd->current_counted = false;
  if (rd->has_top_k && !res->status) {  // (hand-out order: the records of its rows go behind those of the stripes before)
    TopKStripe s;
    s.n = res->n_rows;
    s.recs.swap(res->top_k_records);
    rd->top_k_stripes.push_back(std::move(s));
  }
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
    } while (!rc && rd->next_stripe < rd->stripe_order.size() && stager_has_room(got.size(), staged_bytes, 0));
    std::vector<orcgpu_result*> res(got.size(), nullptr);
    for (auto& r : res) r = reader_take_spare(rd);  // (results the caller is done with are decoded into again: their arenas and pinned host copies stay)
    const double t2 = now();
    if (!rc && !got.empty()) rc = orcgpu_decode_staged(ctx, got.data(), (uint32_t)got.size(), res.data());
    const double t3 = now();
    for (size_t k = 0; k < got.size(); k++) rc = reader_finish_decoded(rd, got[k], res[k], false, rc);
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
  reader_make_current(rd, rd->serial_q.front());
  rd->serial_q.pop_front();
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
      rd->cv_staged_room.wait(g, [rd] { return rd->stop || stager_has_room(rd->staged_q.size(), staged_queue_bytes(rd), rd->prefetch); });
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
    if (rc) rd->stager_err = ctx_err_text(rd->ctx);
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
        return decoder_should_wake(rd->staged_q.size(), staged_queue_bytes(rd), pieces_only);
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
      while (!rd->staged_q.empty() && joins_group(group.size(), group_bytes, orcgpu_staged_bytes(rd->staged_q.front()), room)) {
        group_bytes += orcgpu_staged_bytes(rd->staged_q.front());
        group.push_back(rd->staged_q.front());
        rd->staged_q.pop_front();
        results.push_back(reader_take_spare(rd));  // (a result the caller has given back is decoded into again: no allocations in steady state)
      }
    }
    rd->cv_staged_room.notify_all();
    rc = orcgpu_decode_staged(ctx, group.data(), (uint32_t)group.size(), results.data());
    for (size_t k = 0; k < group.size(); k++) rc = reader_finish_decoded(rd, group[k], results[k], true, rc);
    if (rc) {
      err = ctx_err_text(ctx);
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
