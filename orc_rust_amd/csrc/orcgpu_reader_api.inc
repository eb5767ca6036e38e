// orcgpu_reader_api.inc -- the C ABI of the file reader (include/orcgpu.h: orcgpu_reader_*): the builder's setters, next_batch on
// the host and the device path, the aggregate call.  The reader behind it: orcgpu_reader.inc.
#include "orcgpu_dictionary_names.inc"
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
int orcgpu_reader_filter_overflow_rows(const orcgpu_reader* rd, uint64_t* rows) {
  if (!rd || !rows) return ORCGPU_INVALID_ARGUMENT;
  *rows = rd->filter_overflow.load();
  return ORCGPU_OK;
}
int orcgpu_reader_set_computed_columns(orcgpu_reader* rd, const char* const* names, const orcgpu_agg_expr* exprs, uint32_t n) {
  if (!rd) return ORCGPU_INVALID_ARGUMENT;
  if (rd->built) {
    set_err(rd->ctx, "computed columns: set after the reader has been built (its first batch, column count or drain)");
    return ORCGPU_INVALID_ARGUMENT;
  }
  // what needs no column of the file is refused here, the rest when the reader is built: the projection is known then
  char err[256] = "";
  if (const int rc = orcgpu_host::computed_check_names(names, n, nullptr, 0, err, sizeof(err))) {
    set_err(rd->ctx, "%s", err);
    return rc;
  }
  for (uint32_t k = 0; k < n; k++)
    if (!exprs || (exprs[k].n_nodes && !exprs[k].nodes)) {
      set_err(rd->ctx, "computed columns: an expression without its nodes");
      return ORCGPU_INVALID_ARGUMENT;
    }
  rd->computed_specs.assign(n, {});
  for (uint32_t k = 0; k < n; k++) {
    orcgpu_reader::ComputedSpec& s = rd->computed_specs[k];
    s.name = names[k];
    // (one node past the limit is kept, so that the plan compiler refuses the expression with its message)
    for (uint32_t x = 0; x < exprs[k].n_nodes && x <= ORCGPU_AGG_EXPR_MAX_NODES; x++) {
      const orcgpu_agg_expr_node& nd = exprs[k].nodes[x];
      orcgpu_reader::AggSpec::ExprNode e;
      e.n = nd;
      e.has_column = nd.column != nullptr;
      if (e.has_column) e.column = nd.column;
      e.has_s = nd.s != nullptr && nd.s_len <= 64;
      if (e.has_s) e.s.assign(nd.s, nd.s_len);
      else e.n.s_len = 0;
      s.expr.push_back(std::move(e));
    }
  }
  rd->has_computed = true;
  return ORCGPU_OK;
}
int orcgpu_reader_computed_overflow_rows(const orcgpu_reader* rd, uint64_t* rows) {
  if (!rd || !rows) return ORCGPU_INVALID_ARGUMENT;
  *rows = rd->computed_overflow.load();
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
  rd->opt.project_all = false;
  rd->opt.projected_names.clear();
  for (uint32_t i = 0; i < n; i++) rd->opt.projected_names.emplace_back(names[i]);
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
  rd->opt.dict_names.swap(list);
  return ORCGPU_OK;
}
int orcgpu_reader_set_projection_roots(orcgpu_reader* rd, const uint32_t* roots, uint32_t n) {
  if (!rd || rd->built || (n && !roots)) return ORCGPU_INVALID_ARGUMENT;
  rd->opt.project_all = false;
  rd->opt.by_index = true;
  rd->opt.projected_roots.assign(roots, roots + n);
  return ORCGPU_OK;
}
int orcgpu_reader_set_schema(orcgpu_reader* rd, const struct ArrowSchema* schema) {
  if (!rd || rd->built || !schema || !schema->format || strcmp(schema->format, "+s") != 0) return ORCGPU_INVALID_ARGUMENT;
  rd->opt.has_schema = true;
  rd->opt.schema_tree.clear();
  std::function<void(const ArrowSchema*, orcgpu_host::SchemaNode&)> walk = [&](const ArrowSchema* c, orcgpu_host::SchemaNode& nd) {
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
    rd->opt.schema_tree.emplace_back();
    walk(c, rd->opt.schema_tree.back());
  }
  return ORCGPU_OK;
}
int orcgpu_reader_set_shard(orcgpu_reader* rd, uint32_t rank, uint32_t world, int mode) {
  if (!rd || rd->built || !world || rank >= world || (mode != ORCGPU_SHARD_STRIPES && mode != ORCGPU_SHARD_COLUMNS)) return ORCGPU_INVALID_ARGUMENT;
  rd->opt.shard_rank = rank;
  rd->opt.shard_world = world;
  rd->opt.shard_mode = mode;
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
  rd->opt.ts_arrow_target = arrow_target;
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
  return (uint32_t)rd->proj.names.size();
}
const char* orcgpu_reader_column_name(orcgpu_reader* rd, uint32_t i) {
  if (!rd || orcgpu_host::reader_build(rd) || i >= rd->proj.names.size()) return nullptr;
  return rd->proj.names[i].c_str();
}

int orcgpu_index_entry(const orcgpu_column* column, int has_present, int compressed, const uint64_t* positions, uint32_t n_positions,
                       int32_t kind, orcgpu_stream_entry* out) {
  if (!column || (n_positions && !positions) || !out) return ORCGPU_INVALID_ARGUMENT;
  orcgpu_host::EntrySplit sp;
  if (!orcgpu_host::split_index_entry(column->orc_type, column->encoding, has_present != 0, compressed != 0, positions, n_positions, sp)) return ORCGPU_OUT_OF_SPEC;
  // (INVALID_ARGUMENT: a stream without positions (dictionaries), or one the column does not have)
  return orcgpu_host::stream_entry(sp, kind, has_present != 0, *out) ? ORCGPU_OK : ORCGPU_INVALID_ARGUMENT;
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
  if (rd->has_top_k && !rd->top_k_ready) {  // (the sort keys likewise: refused before anything of the file is read)
    const int rc = orcgpu_host::reader_compile_top_k(rd);
    if (rc) {
      rd->filter_failed = true;
      rd->next_stripe = rd->stripe_order.size();
      return rc;
    }
    rd->top_k_ready = true;
  }
  return ORCGPU_OK;
}
static int reader_next(orcgpu_reader* rd, struct ArrowArray* out_array, struct ArrowDeviceArray* out_device, struct ArrowSchema* out_schema) {
  if (!rd || (!out_array && !out_device) || !out_schema) return ORCGPU_INVALID_ARGUMENT;
  if (rd->has_aggs) {
    set_err(rd->ctx, "this reader aggregates (orcgpu_reader_set_aggregates): call orcgpu_reader_aggregate, it hands out no batches");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (rd->has_collect) {
    set_err(rd->ctx, "this reader collected keys (orcgpu_reader_collect_keys): it hands out no batches");
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
    for (size_t k : rd->proj.roots()) {
      const int kind = rd->md.types[rd->proj.cols[k].id].kind;
      if (orcgpu_host::is_nested_kind(kind) && !rd->device_refused) {
        rd->device_refused = true;
        rd->device_refused_name = rd->proj.names[rd->proj.cols[k].root];
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
        if (out_device) return export_batch_device_named(rd->ctx, rd->current, rd->next_batch++, out_device, out_schema, &rd->proj.names);
        rc = export_batch_named(rd->ctx, rd->current, rd->next_batch++, out_array, out_schema, &rd->proj.names);
        if (!rd->current_counted) {  // (the stripe's copy back has been started by now, by the worker or by this export)
          rd->d2h_bytes += rd->current->d2h_bytes;
          rd->current_counted = true;
        }
        return rc;
      }
    }
    rc = reader_next_stripe(rd);  // (ORCGPU_END_OF_FILE: every stripe has been handed out)
    if (rc == ORCGPU_END_OF_FILE) rd->top_k_eof = true;
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
    orcgpu_host::ctx_err_put(rd->ctx, item.err);
    return item.rc;
  }
  orcgpu_host::reader_make_current(rd, item.res);
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
int orcgpu_reader_set_top_k(orcgpu_reader* rd, const orcgpu_sort_key* keys, uint32_t n_keys, uint32_t k) {
  if (!rd || rd->built) return ORCGPU_INVALID_ARGUMENT;
  if (rd->has_aggs) {
    set_err(rd->ctx, "top-k: this reader aggregates (orcgpu_reader_set_aggregates): it hands out no rows to select from");
    return ORCGPU_INVALID_ARGUMENT;
  }
  // what needs no column is refused here, the rest with the first batch: the columns are known once the reader is built
  orcgpu_host::TopKPlan plan;
  const int rc = orcgpu_host::top_k_compile(keys, n_keys, k, nullptr, nullptr, 0, plan);
  if (rc && (!keys || !n_keys || n_keys > ORCGPU_TOP_K_MAX_KEYS || !k || k > ORCGPU_TOP_K_MAX)) {
    set_err(rd->ctx, "%s", plan.err);
    return rc;
  }
  for (uint32_t q = 0; q < n_keys; q++)
    if (!keys[q].column) {
      set_err(rd->ctx, "top-k: a sort key without a column name");
      return ORCGPU_INVALID_ARGUMENT;
    }
  rd->top_k_keys.clear();
  for (uint32_t q = 0; q < n_keys; q++) rd->top_k_keys.push_back({keys[q].column, keys[q].descending ? 1u : 0u, keys[q].nulls_first ? 1u : 0u});
  rd->top_k_k = k;
  rd->has_top_k = true;
  return ORCGPU_OK;
}
int orcgpu_reader_top_k_order(orcgpu_reader* rd, uint64_t* positions, uint64_t cap, uint64_t* n) {
  if (!rd || !n) return ORCGPU_INVALID_ARGUMENT;
  *n = 0;
  if (!rd->has_top_k) {
    set_err(rd->ctx, "top-k: orcgpu_reader_top_k_order needs orcgpu_reader_set_top_k before the first call");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (!rd->top_k_eof || !rd->top_k_ready) {
    set_err(rd->ctx, "top-k: orcgpu_reader_top_k_order is legal once next_batch has returned ORCGPU_END_OF_FILE");
    return ORCGPU_INVALID_ARGUMENT;
  }
  const int rc = orcgpu_host::top_k_merge(rd->top_k_stripes, rd->top_k_plan.keys.len, rd->top_k_k, positions, cap, n);
  if (rc) set_err(rd->ctx, "top-k: room for %llu positions, the answer holds %llu", (unsigned long long)cap, (unsigned long long)*n);
  return rc;
}
int orcgpu_reader_set_aggregates(orcgpu_reader* rd, const orcgpu_agg_spec* specs, uint32_t n_specs) {
  return orcgpu_reader_set_aggregate_exprs(rd, specs, nullptr, n_specs);
}
int orcgpu_reader_set_aggregate_exprs(orcgpu_reader* rd, const orcgpu_agg_spec* specs, const orcgpu_agg_expr* exprs, uint32_t n_specs) {
  if (!rd || rd->built || !specs || !n_specs || n_specs > ORCGPU_AGG_MAX) return ORCGPU_INVALID_ARGUMENT;
  if (rd->has_top_k) {
    set_err(rd->ctx, "aggregate: this reader selects the top k rows (orcgpu_reader_set_top_k): it does not aggregate as well");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (exprs)
    for (uint32_t k = 0; k < n_specs; k++)
      if (exprs[k].n_nodes && !exprs[k].nodes) return ORCGPU_INVALID_ARGUMENT;
  rd->agg_specs.assign(n_specs, {});
  for (uint32_t k = 0; k < n_specs; k++) {
    orcgpu_reader::AggSpec& s = rd->agg_specs[k];
    s.op = specs[k].op;
    s.has_column = specs[k].column != nullptr;
    s.has_column2 = specs[k].column2 != nullptr;
    if (s.has_column) s.column = specs[k].column;
    if (s.has_column2) s.column2 = specs[k].column2;
    // (one node past the limit is kept, so that the plan compiler refuses the expression with its message; what a literal's bytes
    // mean is the compiler's to say too: 16 for a Decimal)
    for (uint32_t x = 0; exprs && x < exprs[k].n_nodes && x <= ORCGPU_AGG_EXPR_MAX_NODES; x++) {
      const orcgpu_agg_expr_node& n = exprs[k].nodes[x];
      orcgpu_reader::AggSpec::ExprNode e;
      e.n = n;
      e.has_column = n.column != nullptr;
      if (e.has_column) e.column = n.column;
      e.has_s = n.s != nullptr && n.s_len <= 64;
      if (e.has_s) e.s.assign(n.s, n.s_len);
      else e.n.s_len = 0;  // (no bytes are kept: no length either)
      s.expr.push_back(std::move(e));
    }
  }
  rd->has_aggs = true;
  return ORCGPU_OK;
}
int orcgpu_reader_set_aggregate_filters(orcgpu_reader* rd, const orcgpu_agg_filter* filters, uint32_t n_specs) {
  if (!rd || rd->built || !rd->has_aggs || n_specs != rd->agg_specs.size()) return ORCGPU_INVALID_ARGUMENT;
  for (uint32_t k = 0; filters && k < n_specs; k++)
    if (filters[k].n_nodes && !filters[k].nodes) return ORCGPU_INVALID_ARGUMENT;
  for (uint32_t k = 0; k < n_specs; k++) {
    rd->agg_specs[k].filter.clear();
    if (filters && filters[k].n_nodes) rd->agg_specs[k].filter = orcgpu_host::copy_predicate(filters[k].nodes, filters[k].n_nodes);
  }
  return ORCGPU_OK;
}
// What the two drains share.  reader_drain_begin: a reader is drained once, and built first; from then on whatever comes of it ends
// the reader as an error ends an iterator.  reader_drain: rc is what the compile steps gave; then the filter, then every stripe in
// stripe order handed to merge_stripe (rd->current: its status ends the loop).  ORCGPU_OK: every stripe has been merged.
static int reader_drain_begin(orcgpu_reader* rd) {
  if (rd->aggs_done) return ORCGPU_END_OF_FILE;
  const int rc = orcgpu_host::reader_build(rd);
  if (!rc) rd->aggs_done = true;
  return rc;
}
static int reader_drain(orcgpu_reader* rd, int rc, const std::function<int()>& merge_stripe) {
  if (!rc) rc = reader_ready_filter(rd);
  if (rc) {
    rd->next_stripe = rd->stripe_order.size();
    return rc;
  }
  while (!(rc = reader_next_stripe(rd)))
    if ((rc = merge_stripe())) break;
  if (rc == ORCGPU_END_OF_FILE) return ORCGPU_OK;
  orcgpu_host::reader_stop_worker(rd);
  rd->next_stripe = rd->stripe_order.size();
  return rc;
}
// Drains the reader: every stripe's records, merged in stripe order, then the values
int orcgpu_reader_aggregate(orcgpu_reader* rd, orcgpu_agg_value* out) {
  if (!rd || !out) return ORCGPU_INVALID_ARGUMENT;
  if (!rd->has_aggs) {
    set_err(rd->ctx, "orcgpu_reader_aggregate needs orcgpu_reader_set_aggregates before the first call");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (rd->has_group) {
    set_err(rd->ctx, "this reader groups its aggregates (orcgpu_reader_set_group_by): call orcgpu_reader_aggregate_groups");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (const int rc = reader_drain_begin(rd)) return rc;
  int rc = orcgpu_host::reader_compile_aggs(rd);
  const std::vector<AggInsn>& insns = rd->agg_plan.insns;
  std::vector<AggPartial> total(insns.size(), AggPartial{});
  rc = reader_drain(rd, rc, [&]() -> int {
    const std::vector<AggPartial>& part = rd->current->agg_records;
    if (part.size() != insns.size() + 1) {
      set_err(rd->ctx, "aggregate: a stripe came without its records");
      return ORCGPU_UNEXPECTED;
    }
    for (size_t k = 0; k < insns.size(); k++) orcgpu_host::agg_merge(insns[k], total[k], part[k]);
    return ORCGPU_OK;
  });
  if (rc) return rc;
  for (size_t k = 0; k < insns.size(); k++) orcgpu_host::agg_finish(insns[k], total[k], &out[k]);
  return ORCGPU_OK;
}
int orcgpu_reader_set_group_by(orcgpu_reader* rd, const char* const* key_columns, uint32_t n_keys) {
  if (!rd || rd->built || !key_columns || !n_keys || n_keys > ORCGPU_GROUP_MAX_KEYS) return ORCGPU_INVALID_ARGUMENT;
  for (uint32_t k = 0; k < n_keys; k++)
    if (!key_columns[k]) return ORCGPU_INVALID_ARGUMENT;
  rd->group_keys.assign(key_columns, key_columns + n_keys);
  rd->has_group = true;
  return ORCGPU_OK;
}
int orcgpu_reader_set_group_limits(orcgpu_reader* rd, uint32_t max_groups, uint32_t max_total) {
  if (!rd || rd->built) return ORCGPU_INVALID_ARGUMENT;
  char err[256];
  const int rc = orcgpu_host::group_limits(max_groups, max_total, &rd->group_max, &rd->group_max_total, err, sizeof(err));  // (0: the default)
  if (rc) set_err(rd->ctx, "%s", err);
  return rc;
}
// Drains the reader: every stripe's groups, merged by key in stripe order, then the keys and the values
int orcgpu_reader_aggregate_groups(orcgpu_reader* rd, orcgpu_groups** out) {
  if (out) *out = nullptr;
  if (!rd || !out) return ORCGPU_INVALID_ARGUMENT;
  if (!rd->has_group) {
    set_err(rd->ctx, "orcgpu_reader_aggregate_groups needs orcgpu_reader_set_group_by before the first call");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (const int rc = reader_drain_begin(rd)) return rc;
  int rc = ORCGPU_OK;
  if (!rd->has_aggs) {
    set_err(rd->ctx, "group by: orcgpu_reader_set_group_by without orcgpu_reader_set_aggregates");
    rc = ORCGPU_INVALID_ARGUMENT;
  }
  if (!rc) rc = orcgpu_host::reader_compile_group(rd);
  if (!rc) rc = orcgpu_host::reader_compile_aggs(rd);
  std::vector<AggInsn> insns = rd->agg_plan.insns;
  const uint32_t n_specs = (uint32_t)insns.size();
  insns.push_back(AggInsn{});  // (the group's kept row count: AK_COUNT_ROWS)
  const size_t nk = rd->group_plan.keys.size(), ni = insns.size();
  orcgpu_host::GroupSet total;
  total.n_keys = (uint32_t)nk;
  total.n_insn = (uint32_t)ni;
  rc = reader_drain(rd, rc, [&]() -> int {
    const orcgpu_result* res = rd->current;
    if (res->grp_keys.size() % nk || res->grp_vals.size() != res->grp_keys.size() / nk * ni) {
      set_err(rd->ctx, "group by: a stripe came without its groups");
      return ORCGPU_UNEXPECTED;
    }
    char err[256];
    const int mrc = orcgpu_host::group_merge(rd->group_plan, insns, total, res->grp_keys.data(), res->grp_vals.data(), (uint32_t)(res->grp_keys.size() / nk), err, sizeof(err));
    if (mrc) set_err(rd->ctx, "%s", err);
    return mrc;
  });
  if (rc) return rc;
  orcgpu_groups* g = new orcgpu_groups;
  orcgpu_host::group_finish(rd->group_plan, insns, n_specs, total, *g);
  *out = g;
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
