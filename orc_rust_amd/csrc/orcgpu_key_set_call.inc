// orcgpu_key_set_call.inc -- device-resident key sets at the seam (include/orcgpu.h: orcgpu_key_set_*, orcgpu_result_collect_keys,
// orcgpu_reader_collect_keys).  The arithmetic is orcgpu_key_set.inc (host only), the kernels device/key_set_kernels.hip; the
// filter's call (orcgpu_filter.inc) lends its FilterCall, its workspace, its opening and the front of its pipeline up to the
// evaluation, as it does to the aggregation.
//
// A collect on one decoded result: open -> reserve -> upload -> plane kernels -> filter_eval_kernel (its keep mask and nothing
// after it; without a filter every input row is kept) -> key_set_insert_kernel.  Nothing is fetched and nobody waits: the build's
// ONE wait is the seal's, which fetches the control words behind key_set_seal_kernel.
//
// Who owns the memory: the handle and every FilterPlan that names the sealed table (FilterPlan::holds) share it; the last of them
// frees it.  A plan lives in its reader, or for the length of a result call -- and hipFree waits for the device, so kernels that
// still probe the table have run when it goes.
namespace {
struct KeySetMem {
  DevBuf buf;
  DevBuf values;  // a key map's value planes (orcgpu_key_map.inc); a set: none
  ~KeySetMem() {
    buf.release();
    values.release();
  }
};
}  // namespace

struct orcgpu_key_set {
  orcgpu_ctx* ctx = nullptr;
  uint64_t id = 0;
  uint32_t max_keys = 0, hash_mask = 0xffffffffu;
  orcgpu_host::KeySetLayout lay;
  std::shared_ptr<KeySetMem> mem;
  int state = orcgpu_host::KEY_SET_BUILDING;
  orcgpu_key_set_info info{};
  uint32_t sealed_flags = 0;  // the control words' flags as the seal fetched them (a key map reads its duplicate flag here)
};

orcgpu_host::KeySetRefs ctx_key_set_refs(orcgpu_ctx* ctx) {
  orcgpu_host::KeySetRefs out;
  std::lock_guard<std::mutex> g(ctx->key_sets_m);
  for (auto& kv : ctx->key_sets) {
    const orcgpu_key_set* s = kv.second;
    orcgpu_host::KeySetRef ref;
    ref.id = s->id;
    ref.state = s->state;
    ref.table = (uint64_t)(uintptr_t)s->mem->buf.p;
    ref.bytes = (uint32_t)s->lay.table_bytes;
    ref.n_keys = (uint32_t)s->info.n_keys;
    ref.max_keys = s->max_keys;
    ref.has_null = s->info.has_null != 0;
    ref.hold = s->mem;
    out.push_back(std::move(ref));
  }
  return out;
}

namespace {

int key_set_usable_for_collect(orcgpu_ctx* ctx, const orcgpu_key_set* set) {
  if (set->ctx != ctx) {
    set_err(ctx, "key set: the set belongs to another context");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (set->state != orcgpu_host::KEY_SET_BUILDING) {
    if (set->state == orcgpu_host::KEY_SET_SEALED) set_err(ctx, "key set: the set is sealed: it takes no further keys");
    else set_err(ctx, "key set: the set took more than its limit of %u keys and is unusable", set->max_keys);
    return ORCGPU_INVALID_ARGUMENT;
  }
  return ORCGPU_OK;
}

// The kept rows of `r` -- those `fplan` keeps (null: all of them) -- give the keys of column `col` to `set`.  The result is read,
// never changed.  column_names: the result's columns, for the messages.
int key_set_collect_call(orcgpu_ctx* ctx, const orcgpu_result* r_, const orcgpu_host::FilterPlan* fplan, uint32_t col, orcgpu_key_set* set,
                         const char* const* column_names, uint32_t n_names, uint64_t* rows_seen) {
  static const orcgpu_host::FilterPlan no_filter;
  orcgpu_result* r = const_cast<orcgpu_result*>(r_);  // (what is written is the filter's scratch allocation, never a batch)
  if (rows_seen) *rows_seen = 0;
  if (r->status) return r->status;
  if (col >= r->cols.size()) return ORCGPU_UNEXPECTED;
  const ColumnOut& co = r->cols[col];
  const char* name = col < n_names && column_names ? column_names[col] : "";
  char err[256];
  if (const int rc = orcgpu_host::key_set_column_check(co.orc_type, co.dict_out, co.is_struct || co.is_union || co.is_list || co.elem || co.parent >= 0, name, "key set", err, sizeof(err))) {
    set_err(ctx, "%s", err);
    return rc;
  }
  FilterCall f{ctx, r, fplan ? *fplan : no_filter, column_names, n_names, fplan != nullptr};
  uint64_t seen = 0;
  if (const int rc = filter_open(f, &seen)) return rc;
  const FilterWorkspace ws = filter_workspace(f);
  if (const int rc = filter_reserve(f, ws, ws.bytes, "the key set's build")) return rc;
  if (f.fcols[col].kind != FKIND_INT) {
    set_err(ctx, "key set: column '%s' is not decoded to the integers its keys are taken as", name);
    return ORCGPU_MISMATCHED_SCHEMA;
  }
  if (rows_seen) *rows_seen = seen;
  set->info.rows_seen += seen;
  if (!f.n_in) return ORCGPU_OK;
  if (const int rc = filter_upload(f, ws)) return rc;
  if (f.has_filter)
    if (const int rc = filter_run_eval(f, ws)) return rc;
  const KeptRows rows = filter_kept_rows(f, ws);
  uint8_t* T = set->mem->buf.p;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((ws.n_words + 3) / 4, 16384);
  hipLaunchKernelGGL(key_set_insert_kernel, dim3(blocks), dim3(256), 0, ctx->stream, rows, col, reinterpret_cast<unsigned long long*>(T + set->lay.o_slots), set->lay.n_slots,
                     set->max_keys, set->hash_mask, reinterpret_cast<KeySetControl*>(T + set->lay.o_ctl));
  HIP_TRY(ctx, hipGetLastError());
  return ORCGPU_OK;
}

}  // namespace

namespace orcgpu_host {
// The collect of one decoded (and selected) stripe of a reader, where the aggregation stands otherwise: nothing stays with the
// result.  A stripe whose decode failed ends the call.
int reader_collect_map_result(orcgpu_reader* rd, orcgpu_result* res);  // (orcgpu_key_map.inc)
int reader_collect_result(orcgpu_reader* rd, orcgpu_result* res) {
  if (rd->collect_map) return reader_collect_map_result(rd, res);
  if (res->status) {
    set_err(rd->ctx, "stripe decode failed in batch %u, column %u", res->err_batch, res->err_col);
    return res->status;
  }
  const std::vector<const char*> names = reader_c_strings(rd->proj.names);
  if (names.size() != res->cols.size()) {  // (a flat projection: one result column per root column)
    set_err(rd->ctx, "key set: the result holds %zu columns for %zu projected root columns (a nested column in the projection)", res->cols.size(), names.size());
    return ORCGPU_UNSUPPORTED;
  }
  uint64_t seen = 0;
  const int rc = key_set_collect_call(rd->ctx, res, rd->has_filter ? &rd->filter_plan : nullptr, rd->collect_col, rd->collect_set, names.data(), (uint32_t)names.size(), &seen);
  rd->filter_seen += seen;
  return rc;
}
}  // namespace orcgpu_host

extern "C" {

int orcgpu_key_set_create(orcgpu_ctx* ctx, uint64_t max_keys, orcgpu_key_set** out) {
  static std::atomic<uint64_t> next_id{1};
  if (out) *out = nullptr;
  if (!ctx || !out) return ORCGPU_INVALID_ARGUMENT;
  orcgpu_host::KeySetLayout lay;
  if (!orcgpu_host::key_set_layout(max_keys, lay)) {
    set_err(ctx, "key set: max_keys is %llu (1 .. ORCGPU_KEY_SET_MAX_KEYS = %u)", (unsigned long long)max_keys, ORCGPU_KEY_SET_MAX_KEYS);
    return ORCGPU_INVALID_ARGUMENT;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::unique_ptr<orcgpu_key_set> set(new orcgpu_key_set());
  set->ctx = ctx;
  set->max_keys = (uint32_t)max_keys;
  set->lay = lay;
  set->hash_mask = orcgpu_host::key_set_hash_mask(getenv("ORCGPU_KEY_SET_HASH_BITS"));
  set->mem = std::make_shared<KeySetMem>();
  if (!set->mem->buf.ensure(lay.bytes)) {
    set_err(ctx, "hipMalloc(%llu) for a key set of %llu keys failed", (unsigned long long)lay.bytes, (unsigned long long)max_keys);
    return ORCGPU_HIP_ERROR;
  }
  uint8_t* T = set->mem->buf.p;
  // ORCGPU_POISON, the debugging aid of the decode, over the whole table first: nothing may depend on what the memory held
  const char* poison = getenv("ORCGPU_POISON");
  if (poison && *poison) HIP_TRY(ctx, hipMemsetAsync(T, (int)strtol(poison, nullptr, 0) & 0xFF, lay.bytes, ctx->stream));
  HIP_TRY(ctx, hipMemsetAsync(T + lay.o_slots, 0x80, (size_t)lay.n_slots * 8, ctx->stream));  // every slot free: kKeySetSentinel
  HIP_TRY(ctx, hipMemsetAsync(T + lay.o_ctl, 0, 256, ctx->stream));
  set->id = next_id.fetch_add(1);
  {
    std::lock_guard<std::mutex> g(ctx->key_sets_m);
    ctx->key_sets[set->id] = set.get();
  }
  *out = set.release();
  return ORCGPU_OK;
}

uint64_t orcgpu_key_set_id(const orcgpu_key_set* set) { return set ? set->id : 0; }

void orcgpu_key_set_free(orcgpu_key_set* set) {
  if (!set) return;
  {
    std::lock_guard<std::mutex> g(set->ctx->key_sets_m);
    set->ctx->key_sets.erase(set->id);
  }
  (void)hipSetDevice(set->ctx->device);
  delete set;  // (its memory goes with the last plan that names it)
}

int orcgpu_key_set_seal(orcgpu_key_set* set, orcgpu_key_set_info* info) {
  if (!set) return ORCGPU_INVALID_ARGUMENT;
  orcgpu_ctx* ctx = set->ctx;
  if (info) *info = orcgpu_key_set_info{};
  if (set->state == orcgpu_host::KEY_SET_BUILDING) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint8_t* T = set->mem->buf.p;
    const KeySetControl* d_ctl = reinterpret_cast<const KeySetControl*>(T + set->lay.o_ctl);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((set->lay.n_slots / 64 + 3) / 4, 16384);
    hipLaunchKernelGGL(key_set_seal_kernel, dim3(blocks), dim3(256), 0, ctx->stream, T, set->lay.n_slots, set->hash_mask, d_ctl, 0u);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(key_set_seal_kernel, dim3(1), dim3(64), 0, ctx->stream, T, set->lay.n_slots, set->hash_mask, d_ctl, 1u);
    HIP_TRY(ctx, hipGetLastError());
    // ---- the build's one wait: the key count and the flags ----
    KeySetControl ctl{};
    HIP_TRY(ctx, hipMemcpyAsync(&ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const bool over = (ctl.flags & KEY_SET_OVERFLOW) || ctl.n_keys > set->max_keys;
    {
      std::lock_guard<std::mutex> g(ctx->key_sets_m);  // (ctx_key_set_refs reads these)
      set->info.n_keys = over ? 0 : ctl.n_keys;
      set->info.has_null = !over && (ctl.flags & KEY_SET_HAS_NULL) ? 1 : 0;
      set->sealed_flags = ctl.flags;
      set->state = over ? orcgpu_host::KEY_SET_FAILED : orcgpu_host::KEY_SET_SEALED;
    }
  }
  if (set->state == orcgpu_host::KEY_SET_FAILED) {
    set_err(ctx, "key set: more than max_keys = %u distinct keys arrived (orcgpu_key_set_create sets the limit): the set is unusable", set->max_keys);
    return ORCGPU_UNSUPPORTED;
  }
  if (info) *info = set->info;
  return ORCGPU_OK;
}

int orcgpu_result_collect_keys(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes, const char* const* column_names,
                               uint32_t n_columns, const char* column, orcgpu_key_set* set) {
  if (!ctx || !r || (n_nodes && !nodes) || !column_names || !n_columns || !column || !set) return ORCGPU_INVALID_ARGUMENT;
  if (r->status) return r->status;
  if (n_columns != r->cols.size()) {
    set_err(ctx, "key set: %u column names for a result of %zu columns", n_columns, r->cols.size());
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (const int rc = key_set_usable_for_collect(ctx, set)) return rc;
  uint32_t col = n_columns;
  for (uint32_t k = 0; k < n_columns && col == n_columns; k++)
    if (column_names[k] && strcmp(column_names[k], column) == 0) col = k;
  if (col == n_columns) {
    set_err(ctx, "key set: column '%s' is not a projected root column", column);
    return ORCGPU_INVALID_ARGUMENT;
  }
  orcgpu_host::FilterPlan fplan;
  if (n_nodes)
    if (const int rc = result_compile_filter(ctx, r, nodes, n_nodes, column_names, fplan)) return rc;
  return key_set_collect_call(ctx, r, n_nodes ? &fplan : nullptr, col, set, column_names, n_columns, nullptr);
}

// Drains the reader: every stripe's kept keys go into the set where the stripe lies
int orcgpu_reader_collect_keys(orcgpu_reader* rd, const char* column, orcgpu_key_set* set) {
  if (!rd || !column || !set) return ORCGPU_INVALID_ARGUMENT;
  if (rd->has_aggs || rd->has_top_k) {
    set_err(rd->ctx, "key set: this reader %s: it collects no keys as well", rd->has_aggs ? "aggregates (orcgpu_reader_set_aggregates)" : "selects the top k rows (orcgpu_reader_set_top_k)");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (rd->current || rd->next_stripe || rd->worker_started) {
    if (rd->aggs_done) return ORCGPU_END_OF_FILE;
    set_err(rd->ctx, "key set: this reader has handed out batches: orcgpu_reader_collect_keys drains a reader from its start");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (const int rc = key_set_usable_for_collect(rd->ctx, set)) return rc;
  if (const int rc = reader_drain_begin(rd)) return rc;
  int rc = ORCGPU_OK;
  {
    std::vector<const char*> names;
    std::vector<orcgpu_host::AggCol> cols;
    orcgpu_host::reader_describe_roots(rd, names, cols);
    size_t col = names.size();
    for (size_t k = 0; k < names.size() && col == names.size(); k++)
      if (strcmp(names[k], column) == 0) col = k;
    if (col == names.size()) {
      set_err(rd->ctx, "key set: column '%s' is not a projected root column", column);
      rc = ORCGPU_INVALID_ARGUMENT;
    } else {
      char err[256];
      rc = orcgpu_host::key_set_column_check(cols[col].d.orc_type, cols[col].d.dict_out, cols[col].nested, column, "key set", err, sizeof(err));
      if (rc) set_err(rd->ctx, "%s", err);
    }
    rd->collect_col = (uint32_t)col;
  }
  rd->collect_set = set;
  rd->has_collect = true;
  return reader_drain(rd, rc, []() -> int { return ORCGPU_OK; });
}

}  // extern "C"
