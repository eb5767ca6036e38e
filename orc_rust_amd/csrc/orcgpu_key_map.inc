// orcgpu_key_map.inc -- key maps at the seam (include/orcgpu.h: orcgpu_key_map_*, orcgpu_reader_collect_map,
// orcgpu_result_collect_map) and the lookup columns' two entry points (orcgpu_reader_set_lookup_columns,
// orcgpu_result_lookup_columns).  The arithmetic and every refusal of the lookup columns: orcgpu_lookup_plan.inc (host only); the
// kernels: device/key_map_kernels.hip; the decode call's side: orcgpu_lookup.inc.
//
// A key map IS a key set -- the handle holds one, registered with the context under its id, so that ORCGPU_PRED_IN_SET names a
// sealed map as it names a set and the seal runs the set's kernels -- plus the value planes, allocated by the first collect (the
// value kinds are known then) into the set's shared memory block (KeySetMem::values).
//
// A collect on one decoded result is the set's: open -> reserve -> upload -> plane kernels -> filter_eval_kernel ->
// key_map_insert_kernel, whose value table lies behind the filter's workspace.  Nothing is fetched and nobody waits: the build's ONE
// wait is the seal's.
//
// Who owns the memory: the handle, every FilterPlan that names the sealed table, and every reader with lookup columns on the map
// (LookupMapRef::hold, copied when the columns are set) share it; the last of them frees it.

struct orcgpu_key_map {
  orcgpu_key_set set;
  bool has_schema = false;  // the first collect has fixed the values
  uint32_t n_values = 0;
  orcgpu_host::KeyMapValue values[kKeyMapMaxValues];
  orcgpu_host::KeyMapPlanes planes;
  bool duplicate = false;   // sealed and refused: a key came twice
};

namespace {

int key_map_usable_for_collect(orcgpu_ctx* ctx, const orcgpu_key_map* map) {
  if (map->set.ctx != ctx) {
    set_err(ctx, "key map: the map belongs to another context");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (map->set.state != orcgpu_host::KEY_SET_BUILDING) {
    if (map->set.state == orcgpu_host::KEY_SET_SEALED) set_err(ctx, "key map: the map is sealed: it takes no further keys");
    else set_err(ctx, "key map: the map's seal failed (%s) and it is unusable", map->duplicate ? "duplicate key" : "more than max_keys keys");
    return ORCGPU_INVALID_ARGUMENT;
  }
  return ORCGPU_OK;
}

orcgpu_host::LookupMapRef key_map_ref(orcgpu_ctx* ctx, const orcgpu_key_map* map) {
  orcgpu_host::LookupMapRef ref;
  std::lock_guard<std::mutex> g(map->set.ctx->key_sets_m);
  ref.id = map->set.id;
  ref.state = map->set.state;
  ref.same_ctx = map->set.ctx == ctx;
  ref.duplicate = map->duplicate;
  ref.table = (uint64_t)(uintptr_t)map->set.mem->buf.p;
  ref.table_bytes = (uint32_t)map->set.lay.table_bytes;
  ref.n_slots = map->set.lay.n_slots;
  ref.n_values = map->n_values;
  for (uint32_t k = 0; k < map->n_values; k++) ref.values[k] = map->values[k];
  ref.planes = (uint64_t)(uintptr_t)map->set.mem->values.p;
  ref.lay = map->planes;
  ref.hold = map->set.mem;
  return ref;
}

// The values of this collect against the map: the first collect fixes them and allocates the planes, a later one must agree
int key_map_fix_values(orcgpu_ctx* ctx, orcgpu_key_map* map, const orcgpu_host::KeyMapValue* values, uint32_t n) {
  if (map->has_schema) {
    bool same = n == map->n_values;
    for (uint32_t k = 0; same && k < n; k++) same = values[k] == map->values[k];
    if (same) return ORCGPU_OK;
    set_err(ctx, "key map: this collect's value columns (their count, kinds, precision or scale) differ from those of the map's first collect");
    return ORCGPU_MISMATCHED_SCHEMA;
  }
  orcgpu_host::KeyMapPlanes pl;
  if (!orcgpu_host::key_map_planes(map->set.lay.n_slots, values, n, pl)) return ORCGPU_UNEXPECTED;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!map->set.mem->values.ensure(pl.bytes)) {
    set_err(ctx, "hipMalloc(%llu) for the value planes of a key map of %u keys failed", (unsigned long long)pl.bytes, map->set.max_keys);
    return ORCGPU_HIP_ERROR;
  }
  // ORCGPU_POISON over the planes: an entry is read only where a key owns it, and its owner wrote it
  const char* poison = getenv("ORCGPU_POISON");
  if (poison && *poison) HIP_TRY(ctx, hipMemsetAsync(map->set.mem->values.p, (int)strtol(poison, nullptr, 0) & 0xFF, pl.bytes, ctx->stream));
  map->planes = pl;
  map->n_values = n;
  for (uint32_t k = 0; k < n; k++) map->values[k] = values[k];
  map->has_schema = true;
  return ORCGPU_OK;
}

// The kept rows of `r` -- those `fplan` keeps (null: all of them) -- give the keys of column `col` and, beside each, the values
// of columns vcols[0 .. n_values) to `map`.  The result is read, never changed.
int key_map_collect_call(orcgpu_ctx* ctx, const orcgpu_result* r_, const orcgpu_host::FilterPlan* fplan, uint32_t col, const uint32_t* vcols, uint32_t n_values,
                         orcgpu_key_map* map, const char* const* column_names, uint32_t n_names, uint64_t* rows_seen) {
  static const orcgpu_host::FilterPlan no_filter;
  orcgpu_result* r = const_cast<orcgpu_result*>(r_);  // (what is written is the filter's scratch allocation, never a batch)
  if (rows_seen) *rows_seen = 0;
  if (r->status) return r->status;
  if (col >= r->cols.size() || !n_values || n_values > kKeyMapMaxValues) return ORCGPU_UNEXPECTED;
  auto name_of = [&](uint32_t c) { return c < n_names && column_names ? column_names[c] : ""; };
  auto nested = [](const ColumnOut& co) { return co.is_struct || co.is_union || co.is_list || co.elem || co.parent >= 0; };
  char err[320];
  const ColumnOut& kc = r->cols[col];
  if (const int rc = orcgpu_host::key_set_column_check(kc.orc_type, kc.dict_out, nested(kc), name_of(col), "key map", err, sizeof(err))) {
    set_err(ctx, "%s", err);
    return rc;
  }
  orcgpu_host::KeyMapValue values[kKeyMapMaxValues];
  for (uint32_t k = 0; k < n_values; k++) {
    if (vcols[k] >= r->cols.size()) return ORCGPU_UNEXPECTED;
    const ColumnOut& vc = r->cols[vcols[k]];
    if (const int rc = orcgpu_host::key_map_value_check(vc.orc_type, vc.precision, vc.scale, vc.dict_out, nested(vc), name_of(vcols[k]), values[k], err, sizeof(err))) {
      set_err(ctx, "%s", err);
      return rc;
    }
  }
  if (const int rc = key_map_fix_values(ctx, map, values, n_values)) return rc;
  FilterCall f{ctx, r, fplan ? *fplan : no_filter, column_names, n_names, fplan != nullptr};
  uint64_t seen = 0;
  if (const int rc = filter_open(f, &seen)) return rc;
  const FilterWorkspace ws = filter_workspace(f);
  const uint64_t o_vals = align_up(ws.bytes, 16);
  if (const int rc = filter_reserve(f, ws, o_vals + kKeyMapMaxValues * sizeof(KeyMapValueJob), "the key map's build")) return rc;
  if (f.fcols[col].kind != FKIND_INT) {
    set_err(ctx, "key map: column '%s' is not decoded to the integers its keys are taken as", name_of(col));
    return ORCGPU_MISMATCHED_SCHEMA;
  }
  KeyMapValueJob jobs[kKeyMapMaxValues];
  memset(jobs, 0, sizeof(jobs));
  uint8_t* const V = map->set.mem->values.p;
  for (uint32_t k = 0; k < n_values; k++) {
    const FilterCol& fc = f.fcols[vcols[k]];
    const uint32_t want = values[k].kind == KMV_DEC128 ? (uint32_t)FKIND_DEC128 : values[k].kind == KMV_F64 ? (uint32_t)FKIND_FLOAT : (uint32_t)FKIND_INT;
    const bool width_ok = values[k].kind == KMV_DEC128 ? fc.width == 16 : values[k].kind == KMV_F64 ? (fc.width == 4 || fc.width == 8) : (fc.width == 1 || fc.width == 2 || fc.width == 4 || fc.width == 8);
    if (fc.kind != want || !width_ok) {
      set_err(ctx, "key map: value column '%s' is not decoded to the type it is stored as", name_of(vcols[k]));
      return ORCGPU_MISMATCHED_SCHEMA;
    }
    jobs[k].col = vcols[k];
    jobs[k].kind = values[k].kind;
    jobs[k].plane = V + map->planes.o_values[k];
    jobs[k].valid = V + map->planes.o_valid[k];
  }
  if (rows_seen) *rows_seen = seen;
  map->set.info.rows_seen += seen;
  if (!f.n_in) return ORCGPU_OK;
  if (const int rc = filter_upload(f, ws)) return rc;
  HIP_TRY(ctx, ctx->upload(f.X + o_vals, jobs, sizeof(jobs), ctx->stream));
  if (f.has_filter)
    if (const int rc = filter_run_eval(f, ws)) return rc;
  const KeptRows rows = filter_kept_rows(f, ws);
  uint8_t* T = map->set.mem->buf.p;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((ws.n_words + 3) / 4, 16384);
  hipLaunchKernelGGL(key_map_insert_kernel, dim3(blocks), dim3(256), 0, ctx->stream, rows, f.nc, col, reinterpret_cast<unsigned long long*>(T + map->set.lay.o_slots),
                     map->set.lay.n_slots, map->set.max_keys, map->set.hash_mask, reinterpret_cast<KeySetControl*>(T + map->set.lay.o_ctl),
                     f.at<const KeyMapValueJob>(o_vals), n_values);
  HIP_TRY(ctx, hipGetLastError());
  return ORCGPU_OK;
}

// `column` among `names`: its index, or names.size()
size_t key_map_find(const std::vector<const char*>& names, const char* column) {
  for (size_t k = 0; k < names.size(); k++)
    if (names[k] && column && strcmp(names[k], column) == 0) return k;
  return names.size();
}

// the key and the value names -> their columns among `names`; every refusal that needs no column kind
int key_map_resolve(orcgpu_ctx* ctx, const std::vector<const char*>& names, const char* key_column, const char* const* value_columns, uint32_t n_values, uint32_t* col,
                    std::vector<uint32_t>& vcols) {
  char err[256];
  if (const int rc = orcgpu_host::key_map_check_value_names(value_columns, n_values, err, sizeof(err))) {
    set_err(ctx, "%s", err);
    return rc;
  }
  const size_t kc = key_map_find(names, key_column);
  if (kc == names.size()) {
    set_err(ctx, "key map: column '%s' is not a projected root column", key_column);
    return ORCGPU_INVALID_ARGUMENT;
  }
  *col = (uint32_t)kc;
  vcols.clear();
  for (uint32_t k = 0; k < n_values; k++) {
    const size_t vc = key_map_find(names, value_columns[k]);
    if (vc == names.size()) {
      set_err(ctx, "key map: value column '%s' is not a projected root column", value_columns[k]);
      return ORCGPU_INVALID_ARGUMENT;
    }
    vcols.push_back((uint32_t)vc);
  }
  return ORCGPU_OK;
}

// the specs as given -> the plan's input, every map looked at now (a null map stays null: the plan refuses it by name)
void lookup_view_specs(orcgpu_ctx* ctx, const orcgpu_lookup_spec* specs, uint32_t n, std::vector<orcgpu_host::LookupMapRef>& refs, std::vector<orcgpu_host::LookupSpec>& out) {
  refs.resize(n);
  out.resize(n);
  for (uint32_t k = 0; k < n; k++) {
    if (specs[k].map) refs[k] = key_map_ref(ctx, specs[k].map);
    out[k].name = specs[k].name;
    out[k].key_column = specs[k].key_column;
    out[k].map = specs[k].map ? &refs[k] : nullptr;
    out[k].value = specs[k].value;
  }
}

}  // namespace

namespace orcgpu_host {
// The collect of one decoded (and selected) stripe of a reader into a map, where the set's collect stands otherwise
int reader_collect_map_result(orcgpu_reader* rd, orcgpu_result* res) {
  if (res->status) {
    set_err(rd->ctx, "stripe decode failed in batch %u, column %u", res->err_batch, res->err_col);
    return res->status;
  }
  const std::vector<const char*> names = reader_c_strings(rd->proj.names);
  if (names.size() != res->cols.size()) {  // (a flat projection: one result column per root column)
    set_err(rd->ctx, "key map: the result holds %zu columns for %zu projected root columns (a nested column in the projection)", res->cols.size(), names.size());
    return ORCGPU_UNSUPPORTED;
  }
  uint64_t seen = 0;
  const int rc = key_map_collect_call(rd->ctx, res, rd->has_filter ? &rd->filter_plan : nullptr, rd->collect_col, rd->collect_values.data(), (uint32_t)rd->collect_values.size(),
                                      rd->collect_map, names.data(), (uint32_t)names.size(), &seen);
  rd->filter_seen += seen;
  return rc;
}
}  // namespace orcgpu_host

extern "C" {

int orcgpu_key_map_create(orcgpu_ctx* ctx, uint64_t max_keys, orcgpu_key_map** out) {
  if (out) *out = nullptr;
  if (!ctx || !out) return ORCGPU_INVALID_ARGUMENT;
  // (the set inside the handle is made by the set's own call -- its table, its poison, its id, its place in the context's list --
  // and moved into the handle, which the list then names)
  orcgpu_key_set* set = nullptr;
  if (const int rc = orcgpu_key_set_create(ctx, max_keys, &set)) return rc;
  std::unique_ptr<orcgpu_key_map> map(new orcgpu_key_map());
  {
    std::lock_guard<std::mutex> g(ctx->key_sets_m);
    map->set = *set;
    ctx->key_sets[map->set.id] = &map->set;
  }
  delete set;  // (the struct alone: its memory is shared with the copy)
  *out = map.release();
  return ORCGPU_OK;
}

uint64_t orcgpu_key_map_id(const orcgpu_key_map* map) { return map ? map->set.id : 0; }

void orcgpu_key_map_free(orcgpu_key_map* map) {
  if (!map) return;
  {
    std::lock_guard<std::mutex> g(map->set.ctx->key_sets_m);
    map->set.ctx->key_sets.erase(map->set.id);
  }
  (void)hipSetDevice(map->set.ctx->device);
  delete map;  // (its memory goes with the last plan or reader that names it)
}

int orcgpu_key_map_seal(orcgpu_key_map* map, orcgpu_key_map_info* info) {
  if (!map) return ORCGPU_INVALID_ARGUMENT;
  orcgpu_ctx* ctx = map->set.ctx;
  if (info) *info = orcgpu_key_map_info{};
  if (!map->duplicate) {
    orcgpu_key_set_info si{};
    if (const int rc = orcgpu_key_set_seal(&map->set, &si)) return rc;  // (the one wait; more than max_keys keys: its refusal)
    if (map->set.sealed_flags & KEY_MAP_DUPLICATE) {
      std::lock_guard<std::mutex> g(ctx->key_sets_m);
      map->set.state = orcgpu_host::KEY_SET_FAILED;
      map->set.info.n_keys = 0;
      map->set.info.has_null = 0;
      map->duplicate = true;
    }
  }
  if (map->duplicate) {
    set_err(ctx, "key map: duplicate key: two kept rows of the build side hold the same key (a key map takes unique keys): the map is unusable");
    return ORCGPU_UNSUPPORTED;
  }
  if (info) {
    info->n_keys = map->set.info.n_keys;
    info->rows_seen = map->set.info.rows_seen;
    info->has_null = map->set.info.has_null;
    info->n_values = map->n_values;
    for (uint32_t k = 0; k < map->n_values; k++) {
      info->kind[k] = map->values[k].kind;
      info->precision[k] = map->values[k].precision;
      info->scale[k] = map->values[k].scale;
    }
  }
  return ORCGPU_OK;
}

int orcgpu_result_collect_map(orcgpu_ctx* ctx, const orcgpu_result* r, const orcgpu_predicate_node* nodes, uint32_t n_nodes, const char* const* column_names,
                              uint32_t n_columns, const char* key_column, const char* const* value_columns, uint32_t n_values, orcgpu_key_map* map) {
  if (!ctx || !r || (n_nodes && !nodes) || !column_names || !n_columns || !key_column || !map) return ORCGPU_INVALID_ARGUMENT;
  if (r->status) return r->status;
  if (n_columns != r->cols.size()) {
    set_err(ctx, "key map: %u column names for a result of %zu columns", n_columns, r->cols.size());
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (const int rc = key_map_usable_for_collect(ctx, map)) return rc;
  const std::vector<const char*> names(column_names, column_names + n_columns);
  uint32_t col = 0;
  std::vector<uint32_t> vcols;
  if (const int rc = key_map_resolve(ctx, names, key_column, value_columns, n_values, &col, vcols)) return rc;
  orcgpu_host::FilterPlan fplan;
  if (n_nodes)
    if (const int rc = result_compile_filter(ctx, r, nodes, n_nodes, column_names, fplan)) return rc;
  return key_map_collect_call(ctx, r, n_nodes ? &fplan : nullptr, col, vcols.data(), n_values, map, column_names, n_columns, nullptr);
}

// Drains the reader: every stripe's kept keys and their values go into the map where the stripe lies
int orcgpu_reader_collect_map(orcgpu_reader* rd, const char* key_column, const char* const* value_columns, uint32_t n_values, orcgpu_key_map* map) {
  if (!rd || !key_column || !map) return ORCGPU_INVALID_ARGUMENT;
  if (rd->has_aggs || rd->has_top_k) {
    set_err(rd->ctx, "key map: this reader %s: it collects no map as well", rd->has_aggs ? "aggregates (orcgpu_reader_set_aggregates)" : "selects the top k rows (orcgpu_reader_set_top_k)");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (rd->current || rd->next_stripe || rd->worker_started) {
    if (rd->aggs_done) return ORCGPU_END_OF_FILE;
    set_err(rd->ctx, "key map: this reader has handed out batches: orcgpu_reader_collect_map drains a reader from its start");
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (const int rc = key_map_usable_for_collect(rd->ctx, map)) return rc;
  if (const int rc = reader_drain_begin(rd)) return rc;
  int rc = ORCGPU_OK;
  {
    std::vector<const char*> names;
    std::vector<orcgpu_host::AggCol> cols;
    orcgpu_host::reader_describe_roots(rd, names, cols);
    uint32_t col = 0;
    rc = key_map_resolve(rd->ctx, names, key_column, value_columns, n_values, &col, rd->collect_values);
    char err[320];
    if (!rc) {
      rc = orcgpu_host::key_set_column_check(cols[col].d.orc_type, cols[col].d.dict_out, cols[col].nested, key_column, "key map", err, sizeof(err));
      if (rc) set_err(rd->ctx, "%s", err);
    }
    for (size_t k = 0; !rc && k < rd->collect_values.size(); k++) {
      const orcgpu_host::AggCol& c = cols[rd->collect_values[k]];
      orcgpu_host::KeyMapValue v;
      rc = orcgpu_host::key_map_value_check(c.d.orc_type, 0, c.scale, c.d.dict_out, c.nested, value_columns[k], v, err, sizeof(err));
      if (rc) set_err(rd->ctx, "%s", err);
    }
    rd->collect_col = col;
  }
  rd->collect_map = map;
  rd->collect_set = &map->set;
  rd->has_collect = true;
  return reader_drain(rd, rc, []() -> int { return ORCGPU_OK; });
}

int orcgpu_reader_set_lookup_columns(orcgpu_reader* rd, const orcgpu_lookup_spec* specs, uint32_t n) {
  if (!rd) return ORCGPU_INVALID_ARGUMENT;
  if (rd->built) {
    set_err(rd->ctx, "lookup columns: set after the reader has been built (its first batch, column count or drain)");
    return ORCGPU_INVALID_ARGUMENT;
  }
  // what needs no column of the file is refused here, the rest when the reader is built: the projection is known then
  char err[384] = "";
  std::vector<const char*> names;
  for (uint32_t k = 0; specs && k < n && k <= ORCGPU_LOOKUP_MAX; k++) names.push_back(specs[k].name);
  if (const int rc = orcgpu_host::lookup_check_names(specs ? names.data() : nullptr, n, nullptr, 0, nullptr, 0, err, sizeof(err))) {
    set_err(rd->ctx, "%s", err);
    return rc;
  }
  std::vector<orcgpu_host::LookupMapRef> refs;
  std::vector<orcgpu_host::LookupSpec> view;
  lookup_view_specs(rd->ctx, specs, n, refs, view);
  for (uint32_t k = 0; k < n; k++) {
    int rc = orcgpu_host::lookup_check_map(view[k].map, view[k].name, err, sizeof(err));
    if (!rc && (!view[k].key_column || !view[k].key_column[0])) {
      snprintf(err, sizeof(err), "lookup column '%s' names no probe key column", view[k].name);
      rc = ORCGPU_INVALID_ARGUMENT;
    }
    if (!rc && view[k].value >= view[k].map->n_values) {
      snprintf(err, sizeof(err), "lookup column '%s' names value %u of a key map of %u values", view[k].name, view[k].value, view[k].map->n_values);
      rc = ORCGPU_INVALID_ARGUMENT;
    }
    if (rc) {
      set_err(rd->ctx, "%s", err);
      return rc;
    }
  }
  rd->lookup_specs.assign(n, {});
  for (uint32_t k = 0; k < n; k++) {
    orcgpu_reader::LookupSpecCopy& s = rd->lookup_specs[k];
    s.name = view[k].name;
    s.key_column = view[k].key_column;
    s.map = std::make_shared<orcgpu_host::LookupMapRef>(refs[k]);
    s.value = view[k].value;
  }
  rd->has_lookup = true;
  return ORCGPU_OK;
}

int orcgpu_result_lookup_columns(orcgpu_ctx* ctx, orcgpu_result* r, const orcgpu_lookup_spec* specs, uint32_t n, const char* const* column_names) {
  if (!ctx || !r || !column_names) return ORCGPU_INVALID_ARGUMENT;
  if (r->status) return r->status;
  const uint32_t n_file = (uint32_t)r->cols.size();
  std::vector<orcgpu_host::LookupProjCol> pcols(n_file);
  for (uint32_t c = 0; c < n_file; c++) {
    const ColumnOut& co = r->cols[c];
    if (co.computed) {
      set_err(ctx, "lookup columns: the result already holds lookup or computed columns");
      return ORCGPU_INVALID_ARGUMENT;
    }
    pcols[c].orc_type = co.orc_type;
    pcols[c].dict_read = co.dict_out;
    pcols[c].nested = co.is_struct || co.is_union || co.is_list || co.elem || co.parent >= 0;
  }
  std::vector<orcgpu_host::LookupMapRef> refs;
  std::vector<orcgpu_host::LookupSpec> view;
  if (specs) lookup_view_specs(ctx, specs, std::min<uint32_t>(n, ORCGPU_LOOKUP_MAX + 1), refs, view);
  orcgpu_host::LookupPlan plan;
  if (const int rc = orcgpu_host::lookup_compile(specs ? view.data() : nullptr, n, column_names, n_file, nullptr, 0, column_names, pcols.data(), n_file, plan)) {
    set_err(ctx, "%s", plan.err);
    return rc;
  }
  return result_lookup_columns(ctx, r, plan);
}

}  // extern "C"
