// orcgpu_export.inc -- result inspection, host copies and Arrow C Data Interface export.
//
// Per-batch semantics mirror the reference's RecordBatch assembly (array_decoder/mod.rs:531-564):
// every batch has at most batch_size rows, string offsets restart at 0 per batch
// (string.rs:139-140), the validity buffer is omitted when the batch has no nulls (mod.rs:247-251)
// and the field's `nullable` flag follows (RecordBatch::try_from_iter, mod.rs:552-562).

namespace {

void result_destroy(void* result);  // (orcgpu_export_device.inc)

uint64_t batch_rows(const orcgpu_result* r, uint32_t b) {
  if (r->selected) return r->sel[b].len;
  return std::min<uint64_t>(r->batch, r->n_rows - (uint64_t)b * r->batch);
}

struct ExportPriv {
  HostMirror* mirror = nullptr;    // the pinned host copy the buffers point into (one reference held)
  std::vector<void*> owned;        // malloc'd host buffers
  std::vector<const void*> bufs;   // buffers array
  std::vector<ArrowArray*> kids;
  std::vector<ArrowArray> kid_store;
  std::vector<ArrowArray> dict_store;  // a dictionary-output column: ArrowArray::dictionary (one, or none)
};
struct SchemaPriv {
  std::vector<std::string> strings;
  std::vector<ArrowSchema*> kids;
  std::vector<ArrowSchema> kid_store;
  std::vector<ArrowSchema> dict_store;  // ArrowSchema::dictionary
};

void release_array(ArrowArray* a) {
  if (!a || !a->release) return;
  ExportPriv* p = static_cast<ExportPriv*>(a->private_data);
  if (p) {
    for (auto& k : p->kid_store)
      if (k.release) k.release(&k);
    for (auto& k : p->dict_store)
      if (k.release) k.release(&k);
    for (void* q : p->owned) free(q);
    if (p->mirror) p->mirror->unref();
    delete p;
  }
  a->release = nullptr;
}
void release_schema(ArrowSchema* s) {
  if (!s || !s->release) return;
  SchemaPriv* p = static_cast<SchemaPriv*>(s->private_data);
  if (p) {
    for (auto& k : p->kid_store)
      if (k.release) k.release(&k);
    for (auto& k : p->dict_store)
      if (k.release) k.release(&k);
    delete p;
  }
  s->release = nullptr;
}

std::string arrow_format(const ColumnOut& co) {
  static const char* units = "smun";
  if (co.dict_out) return "i";  // the keys; ArrowSchema::dictionary says "u"
  switch (co.orc_type) {
    case ORCGPU_T_BOOLEAN: return "b";
    case ORCGPU_T_BYTE: return "c";
    case ORCGPU_T_SHORT: return "s";
    case ORCGPU_T_INT: return "i";
    case ORCGPU_T_LONG: return "l";
    case ORCGPU_T_FLOAT: return "f";
    case ORCGPU_T_DOUBLE: return "g";
    case ORCGPU_T_DATE: return "tdD";
    case ORCGPU_T_BINARY: return "z";
    case ORCGPU_T_STRING: case ORCGPU_T_VARCHAR: case ORCGPU_T_CHAR: return "u";
    case ORCGPU_T_TIMESTAMP: return co.ts_unit == 4 ? std::string("d:38,9") : std::string("ts") + units[co.ts_unit] + ":";
    case ORCGPU_T_TIMESTAMP_INSTANT: return co.ts_unit == 4 ? std::string("d:38,9") : std::string("ts") + units[co.ts_unit] + ":UTC";
    case ORCGPU_T_DECIMAL: return "d:" + std::to_string(co.precision) + "," + std::to_string(co.scale);
    default: return "n";
  }
}

}  // namespace

extern "C" {

// Starts bringing the result's Arrow buffers to the host: one hipMemcpyAsync per arena into pinned memory (reused from decode
// to decode unless exported batches still hold the previous copy) on the context's device-to-host stream, behind everything
// enqueued on the decode stream so far.  Does not wait: the next stripe can be staged and decoded meanwhile.
int orcgpu_result_fetch_async(orcgpu_ctx* ctx, orcgpu_result* r) {
  if (!ctx || !r) return ORCGPU_INVALID_ARGUMENT;
  if (r->mirror_valid) return ORCGPU_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!ctx->d2h_stream) {
    HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->d2h_stream, hipStreamNonBlocking));
    HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->d2h_gate, hipEventDisableTiming));
  }
  if (r->mirror && r->mirror->refs.load() > 1) {  // batches exported earlier keep their copy
    r->mirror->unref();
    r->mirror = nullptr;
  }
  if (!r->mirror) r->mirror = new HostMirror();
  HostMirror* m = r->mirror;
  m->wait();  // (an earlier copy into the same pinned memory)
  if (!m->done) HIP_TRY(ctx, hipEventCreateWithFlags(&m->done, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventRecord(ctx->d2h_gate, ctx->stream));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->d2h_stream, ctx->d2h_gate, 0));
  r->d2h_bytes = 0;
  auto pull = [&](uint8_t*& host, size_t& cap, const DevBuf& dev, size_t used) -> int {
    if (!used) return ORCGPU_OK;
    if (cap < used) {
      PinnedPool::get().give(host, cap);
      host = nullptr;
      cap = 0;
      const size_t want = used + used / 8 + 4096;
      if (!PinnedPool::get().take(want, host, cap)) {
        set_err(ctx, "hipHostMalloc(%zu) for the host copy of a result failed", want);
        return ORCGPU_HIP_ERROR;
      }
    }
    // (one copy per arena: cutting it into pieces -- so that the small copies of the decode running beside it would wait less
    // behind it -- changed nothing at 32 MiB and cost throughput below 8 MiB: measured, MI355X)
    HIP_TRY(ctx, hipMemcpyAsync(host, dev.p, used, hipMemcpyDeviceToHost, ctx->d2h_stream));
    r->d2h_bytes += used;
    return ORCGPU_OK;
  };
  if (r->filtered) {  // a row filter's kept rows live in an arena of their own: nothing else crosses the link
    int rc = pull(m->filt, m->filt_cap, r->filt_arena, r->filt_used);
    if (rc) return rc;
  }
  for (int l = 0; l < kMaxLanes && !r->filtered; l++) {
    int rc = pull(m->arena[l], m->arena_cap[l], r->arena[l], r->arena_used[l]);
    if (!rc) rc = pull(m->chars[l], m->chars_cap[l], r->chars[l], r->chars_used[l]);
    if (rc) return rc;
  }
  if (!r->filtered) {
    int rc = pull(m->sel, m->sel_cap, r->sel_arena, r->selected ? r->sel_used : 0);
    if (rc) return rc;
  }
  HIP_TRY(ctx, hipEventRecord(m->done, ctx->d2h_stream));
  m->pending = true;
  r->mirror_valid = true;
  for (auto* sub : r->subs) {  // the elements of List / Map columns
    int rc = orcgpu_result_fetch_async(ctx, sub);
    if (rc) return rc;
    r->d2h_bytes += sub->d2h_bytes;
  }
  return ORCGPU_OK;
}

// ... and the same with the wait: when it returns the host copy is complete (also after orcgpu_result_fetch_async).
int orcgpu_result_fetch(orcgpu_ctx* ctx, orcgpu_result* r) {
  if (!ctx || !r) return ORCGPU_INVALID_ARGUMENT;
  if (!r->mirror_valid) {
    int rc = orcgpu_result_fetch_async(ctx, r);
    if (rc) return rc;
  }
  if (r->mirror && r->mirror->pending) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(r->mirror->done));
    r->mirror->pending = false;
  }
  for (auto* sub : r->subs) {
    int rc = orcgpu_result_fetch(ctx, sub);
    if (rc) return rc;
  }
  return ORCGPU_OK;
}

// (a result that device-resident batches still view only loses its owner here: the last of them frees it, device_hold.h)
void orcgpu_result_free(orcgpu_result* r) {
  if (!r) return;
  if (r->hold) orcgpu_hold::hold_owner_done(r->hold, false);
  else result_destroy(r);
}

int orcgpu_result_status(const orcgpu_result* r, uint32_t* batch, uint32_t* column) {
  if (!r) return ORCGPU_INVALID_ARGUMENT;
  if (batch) *batch = r->err_batch;
  if (column) *column = r->err_col;
  return r->status;
}
uint64_t orcgpu_result_rows(const orcgpu_result* r) { return r ? r->n_rows : 0; }
uint32_t orcgpu_result_batches(const orcgpu_result* r) { return r ? r->n_batches : 0; }  // (selected batches after orcgpu_result_select)
uint64_t orcgpu_result_arrow_bytes(const orcgpu_result* r) { return r ? r->arrow_bytes : 0; }

int orcgpu_result_batch_view(const orcgpu_result* r, uint32_t b, uint32_t c, orcgpu_batch_view* out) {
  if (!r || !out || b >= r->n_batches || c >= r->cols.size()) return ORCGPU_INVALID_ARGUMENT;
  const ColumnOut& co = r->cols[c];
  memset(out, 0, sizeof(*out));
  uint64_t rows = batch_rows(r, b);
  out->length = rows;
  out->null_count = r->selected ? 0 : co.null_counts[b];
  const uint8_t* A = r->filtered ? r->filt_arena.p : r->arena[co.lane].p;  // (a filtered result: uniform batches of the kept rows)
  if (r->selected) {
    // a selected batch: rows [start, start + len) of the stripe.  Fixed-width values and string bytes are used in place
    // (contiguous in the stripe-wide buffers); validity, Boolean bits and offsets were rebuilt by orcgpu_result_select
    const SelBatch& sb = r->sel[b];
    const uint8_t* X = r->sel_arena.p;
    out->null_count = co.sel_nulls.empty() ? 0 : co.sel_nulls[b];
    if (out->null_count) out->validity = X + co.sel_validity_off + (uint64_t)b * r->words_per_batch * 8;
    if (co.is_bool) {
      out->values = X + co.sel_bool_off + (uint64_t)b * r->words_per_batch * 8;
      out->values_bytes = (rows + 7) / 8;
    } else if (co.is_list) {
      // (the batch's offsets, from 0; its elements: sel_char_total[b] of them from sel_char_start[b] on in the sub-result)
      out->offsets = reinterpret_cast<const int32_t*>(X + co.sel_offsets_off) + (uint64_t)b * (r->batch + 1);
    } else if (co.is_string) {
      out->offsets = reinterpret_cast<const int32_t*>(X + co.sel_offsets_off) + (uint64_t)b * (r->batch + 1);
      out->values = (co.values_in_chars ? r->chars[co.lane].p : A) + co.values_off + co.sel_char_start[b];
      out->values_bytes = co.sel_char_total[b];
    } else {
      out->values = A + co.values_off + sb.start * co.width;
      out->values_bytes = rows * co.width;
    }
    return ORCGPU_OK;
  }
  if (out->null_count) out->validity = A + co.validity_off + (uint64_t)b * r->words_per_batch * 8;
  if (co.is_bool) {
    out->values = A + co.values_off + (uint64_t)b * r->words_per_batch * 8;
    out->values_bytes = (rows + 7) / 8;
  } else if (co.is_list) {
    // a List / Map: the batch's offsets (in elements, from 0); the elements are columns of the sub-result, reached through
    // orcgpu_result_export_batch
    out->offsets = reinterpret_cast<const int32_t*>(A + co.offsets_off) + (uint64_t)b * (r->batch + 1);
  } else if (co.is_string) {
    out->offsets = reinterpret_cast<const int32_t*>(A + co.offsets_off) + (uint64_t)b * (r->batch + 1);
    out->values = (co.values_in_chars ? r->chars[co.lane].p : A) + co.values_off + co.char_base[b];
    out->values_bytes = co.char_total[b];
  } else {
    out->values = A + co.values_off + (uint64_t)b * r->batch * co.width;
    out->values_bytes = rows * co.width;
  }
  return ORCGPU_OK;
}

// The stripe's dictionary of a dictionary-output column: where it lies now -- in the decode's arena or, behind a row filter, beside
// the kept rows
int orcgpu_result_dictionary_view(const orcgpu_result* r, uint32_t c, orcgpu_dictionary_view* out) {
  if (!r || !out || c >= r->cols.size()) return ORCGPU_INVALID_ARGUMENT;
  const ColumnOut& co = r->cols[c];
  memset(out, 0, sizeof(*out));
  if (!co.dict_out) return ORCGPU_INVALID_ARGUMENT;
  const uint8_t* A = r->filtered ? r->filt_arena.p : r->arena[co.lane].p;
  if (!co.dict_decoded) return ORCGPU_OK;  // (a stripe without rows decodes nothing: no entries, no buffers)
  out->length = co.dict_len;
  out->offsets = reinterpret_cast<const int32_t*>(A + co.dict_offsets_off);
  out->values = A + co.dict_values_off;
  out->values_bytes = co.dict_bytes;
  return ORCGPU_OK;
}

int orcgpu_result_copy_dictionary(orcgpu_ctx* ctx, const orcgpu_result* r, uint32_t c, int32_t* offsets, void* values) {
  orcgpu_dictionary_view v;
  int rc = orcgpu_result_dictionary_view(r, c, &v);
  if (rc) return rc;
  if (!ctx) return ORCGPU_INVALID_ARGUMENT;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  if (offsets && !v.offsets) offsets[0] = 0;
  if (offsets && v.offsets) HIP_TRY(ctx, hipMemcpy(offsets, v.offsets, (v.length + 1) * 4, hipMemcpyDeviceToHost));
  if (values && v.values_bytes) HIP_TRY(ctx, hipMemcpy(values, v.values, v.values_bytes, hipMemcpyDeviceToHost));
  return ORCGPU_OK;
}

int orcgpu_result_copy_batch(orcgpu_ctx* ctx, const orcgpu_result* r, uint32_t b, uint32_t c, void* values, int32_t* offsets, void* validity) {
  orcgpu_batch_view v;
  int rc = orcgpu_result_batch_view(r, b, c, &v);
  if (rc) return rc;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (values && v.values_bytes) HIP_TRY(ctx, hipMemcpy(values, v.values, v.values_bytes, hipMemcpyDeviceToHost));
  if (offsets && v.offsets) HIP_TRY(ctx, hipMemcpy(offsets, v.offsets, (v.length + 1) * 4, hipMemcpyDeviceToHost));
  if (validity && v.validity) HIP_TRY(ctx, hipMemcpy(validity, v.validity, (v.length + 7) / 8, hipMemcpyDeviceToHost));
  return ORCGPU_OK;
}

static int export_batch_named(orcgpu_ctx* ctx, const orcgpu_result* rc_, uint32_t b, struct ArrowArray* oa, struct ArrowSchema* os,
                              const std::vector<std::string>* names) {
  orcgpu_result* r = const_cast<orcgpu_result*>(rc_);
  if (!ctx || !r || !oa || !os || b >= r->n_batches) return ORCGPU_INVALID_ARGUMENT;
  if (r->status && b >= r->err_batch) {
    set_err(ctx, "batch %u is at or past the failing batch %u", b, r->err_batch);
    return r->status;
  }
  int frc = orcgpu_result_fetch(ctx, r);
  if (frc) return frc;
  HostMirror* m = r->mirror;
  const size_t nc = r->cols.size();
  uint64_t rows = batch_rows(r, b);
  static const uint64_t kEmpty[2] = {0, 0};  // zero-length buffers still need an address
  // One column as an Arrow array + schema (a Struct: its fields below it, array_decoder/struct_decoder.rs:58-78; a List / Map:
  // its elements below it, list.rs:63-87 / map.rs:74-104).  `name`: the field name (root columns: the caller's names or
  // "c<column id>"; fields of Structs: the reader's names or "f<position>"; elements: "item" / "entries", "key", "value").
  // q: the result the column lives in -- the stripe's, or the sub-result of the List / Map above it, whose rows are ALL elements
  // of the stripe in one batch: of those the array shows the `len` elements from `off` on (ArrowArray::offset into the
  // buffers of the whole column; its null count is left to the consumer: -1).
  std::function<void(orcgpu_result*, size_t, const std::string&, bool, uint64_t, uint64_t, ArrowArray&, ArrowSchema&)> build =
      [&](orcgpu_result* q, size_t c, const std::string& name, bool sliced, uint64_t off, uint64_t len, ArrowArray& ka, ArrowSchema& ks) {
    const ColumnOut& co = q->cols[c];
    HostMirror* qm = q->mirror;
    orcgpu_batch_view v;
    memset(&v, 0, sizeof(v));
    if (!sliced) orcgpu_result_batch_view(q, b, (uint32_t)c, &v);
    else if (q->n_batches) orcgpu_result_batch_view(q, 0, (uint32_t)c, &v);  // (no elements at all: nothing to view)
    ExportPriv* kp = new ExportPriv();
    // device view -> the same place in the pinned host copy (no further copy: the batch holds a reference to it)
    auto host_of = [&](const void* dev) -> const void* {
      if (!dev || !qm) return nullptr;
      const uint8_t* d = static_cast<const uint8_t*>(dev);
      const DevBuf& A = q->arena[co.lane];
      const DevBuf& C = q->chars[co.lane];
      if (A.p && d >= A.p && d < A.p + A.cap) return qm->arena[co.lane] + (d - A.p);
      if (C.p && d >= C.p && d < C.p + C.cap) return qm->chars[co.lane] + (d - C.p);
      const DevBuf& X = q->sel_arena;
      if (q->filtered) {
        const DevBuf& F = q->filt_arena;
        return F.p && d >= F.p && d < F.p + F.cap ? qm->filt + (d - F.p) : nullptr;
      }
      if (X.p && d >= X.p && d < X.p + X.cap) return qm->sel + (d - X.p);
      return nullptr;
    };
    auto or_empty = [&](const void* p_) -> const void* { return p_ ? p_ : (const void*)kEmpty; };
    if (qm) {
      kp->mirror = qm;
      qm->refs.fetch_add(1);
    }
    kp->bufs.push_back(v.validity ? host_of(v.validity) : nullptr);
    SchemaPriv* ksp = new SchemaPriv();
    const uint64_t my_len = sliced ? len : rows;
    auto add_kid = [&](orcgpu_result* kq, size_t kc, const std::string& kname, bool ksl, uint64_t koff, uint64_t klen) {
      kp->kid_store.emplace_back();
      ksp->kid_store.emplace_back();
      memset(&kp->kid_store.back(), 0, sizeof(ArrowArray));
      memset(&ksp->kid_store.back(), 0, sizeof(ArrowSchema));
      build(kq, kc, kname, ksl, koff, klen, kp->kid_store.back(), ksp->kid_store.back());
    };
    std::string format = arrow_format(co);
    if (co.is_struct) {
      format = "+s";
      std::vector<size_t> fields;
      for (size_t k = c + 1; k < q->cols.size(); k++)
        if (q->cols[k].parent == (int32_t)c) fields.push_back(k);
      kp->kid_store.reserve(fields.size());
      ksp->kid_store.reserve(fields.size());
      for (size_t f = 0; f < fields.size(); f++) {
        // (field names are kept by the stripe's result, indexed by the staged stripe's columns)
        const size_t orig = q->src_col.empty() ? fields[f] : q->src_col[fields[f]];
        const std::string fname = orig < r->field_names.size() && !r->field_names[orig].empty() ? r->field_names[orig] : "f" + std::to_string(f);
        // (a sliced Struct -- an element of a List -- keeps its fields whole: its own offset applies on top of them)
        add_kid(q, fields[f], fname, sliced, 0, sliced ? q->n_rows : 0);
      }
    } else if (co.is_union) {
      // a sparse Union (schema.rs:560-576, union.rs:126-129): the type ids and one full-length child per arm, no validity of its
      // own -- the arms carry the nulls (the first arm those of the Union itself)
      std::vector<size_t> arms;
      for (size_t k = c + 1; k < q->cols.size(); k++)
        if (q->cols[k].parent == (int32_t)c) arms.push_back(k);
      format = "+us:";
      for (size_t a = 0; a < arms.size(); a++) format += (a ? "," : "") + std::to_string(a);
      kp->bufs.clear();
      kp->bufs.push_back(or_empty(v.values_bytes ? host_of(v.values) : nullptr));
      v.validity = nullptr;
      v.null_count = 0;
      kp->kid_store.reserve(arms.size());
      ksp->kid_store.reserve(arms.size());
      for (size_t a = 0; a < arms.size(); a++) add_kid(q, arms[a], "_union_" + std::to_string(a), sliced, 0, sliced ? q->n_rows : 0);
    } else if (co.is_list) {
      format = co.is_map ? "+m" : "+l";
      kp->bufs.push_back(or_empty(host_of(v.offsets)));
      orcgpu_result* e = co.sub >= 0 && (size_t)co.sub < q->subs.size() ? q->subs[co.sub] : nullptr;
      // the elements of this batch: from char_base[b] on (a sliced List -- a List inside a List -- has ONE batch: its offsets
      // run on from 0 and its elements are all of them)
      uint64_t e_off = 0, e_len = 0;
      if (e) {
        if (!sliced && q->selected) {  // a batch of a row selection: the elements of its rows
          e_off = b < co.sel_char_start.size() ? co.sel_char_start[b] : 0;
          e_len = b < co.sel_char_total.size() ? co.sel_char_total[b] : 0;
        } else if (!sliced) {
          e_off = b < co.char_base.size() ? co.char_base[b] : 0;
          e_len = b < co.char_total.size() ? co.char_total[b] : 0;
        } else {
          e_len = e->n_rows;
        }
      }
      std::vector<size_t> eroots;
      if (e)
        for (size_t k = 0; k < e->cols.size(); k++)
          if (e->cols[k].parent < 0) eroots.push_back(k);
      kp->kid_store.reserve(2);
      ksp->kid_store.reserve(2);
      // (names of the element fields: with_schema's, when it named them)
      auto elem_name = [&](size_t ec, const char* dflt) -> std::string {
        const size_t orig = ec < e->src_col.size() ? e->src_col[ec] : ~(size_t)0;
        return orig < r->field_names.size() && !r->field_names[orig].empty() ? r->field_names[orig] : std::string(dflt);
      };
      if (!co.is_map) {
        if (!eroots.empty()) add_kid(e, eroots[0], elem_name(eroots[0], "item"), true, e_off, e_len);
      } else if (eroots.size() >= 2) {
        // entries: Struct<key not null, value>, no validity (map.rs:96-101)
        kp->kid_store.emplace_back();
        ksp->kid_store.emplace_back();
        ArrowArray& ea = kp->kid_store.back();
        ArrowSchema& es = ksp->kid_store.back();
        ExportPriv* ep = new ExportPriv();
        SchemaPriv* esp = new SchemaPriv();
        ep->kid_store.resize(2);
        esp->kid_store.resize(2);
        for (int kv = 0; kv < 2; kv++) {
          memset(&ep->kid_store[kv], 0, sizeof(ArrowArray));
          memset(&esp->kid_store[kv], 0, sizeof(ArrowSchema));
          build(e, eroots[kv], elem_name(eroots[kv], kv == 0 ? "key" : "value"), true, 0, e->n_rows, ep->kid_store[kv], esp->kid_store[kv]);  // (whole: the offset of `entries` applies on top)
          ep->kids.push_back(&ep->kid_store[kv]);
          esp->kids.push_back(&esp->kid_store[kv]);
        }
        esp->kid_store[0].flags = 0;  // keys are not nullable
        ep->bufs.push_back(nullptr);
        memset(&ea, 0, sizeof(ea));
        ea.length = (int64_t)e_len;
        ea.offset = e_len ? (int64_t)e_off : 0;
        ea.n_buffers = 1;
        ea.buffers = ep->bufs.data();
        ea.n_children = 2;
        ea.children = ep->kids.data();
        ea.release = release_array;
        ea.private_data = ep;
        esp->strings.reserve(2);
        esp->strings.push_back("+s");
        esp->strings.push_back("entries");
        memset(&es, 0, sizeof(es));
        es.format = esp->strings[0].c_str();
        es.name = esp->strings[1].c_str();
        es.flags = 0;
        es.n_children = 2;
        es.children = esp->kids.data();
        es.release = release_schema;
        es.private_data = esp;
      }
    } else if (co.is_string) {
      kp->bufs.push_back(or_empty(host_of(v.offsets)));
      kp->bufs.push_back(or_empty(v.values_bytes ? host_of(v.values) : nullptr));
    } else {
      kp->bufs.push_back(or_empty(v.values_bytes ? host_of(v.values) : nullptr));
    }
    if (co.dict_out) {
      // the stripe's dictionary as a Utf8 array: every batch of the stripe points into the same host copy, which came over with
      // the arena, once, and goes when the last array that refers to it is released (one more reference on the mirror)
      orcgpu_dictionary_view dv;
      memset(&dv, 0, sizeof(dv));
      orcgpu_result_dictionary_view(q, (uint32_t)c, &dv);
      ExportPriv* dp = new ExportPriv();
      if (qm) {
        dp->mirror = qm;
        qm->refs.fetch_add(1);
      }
      dp->bufs.push_back(nullptr);
      dp->bufs.push_back(or_empty(dv.length ? host_of(dv.offsets) : nullptr));
      dp->bufs.push_back(or_empty(dv.values_bytes ? host_of(dv.values) : nullptr));
      kp->dict_store.emplace_back();
      ArrowArray& da = kp->dict_store.back();
      memset(&da, 0, sizeof(da));
      da.length = (int64_t)dv.length;
      da.n_buffers = 3;
      da.buffers = dp->bufs.data();
      da.release = release_array;
      da.private_data = dp;
      SchemaPriv* dsp = new SchemaPriv();
      dsp->strings.reserve(2);
      dsp->strings.push_back("u");
      dsp->strings.push_back("");
      ksp->dict_store.emplace_back();
      ArrowSchema& ds = ksp->dict_store.back();
      memset(&ds, 0, sizeof(ds));
      ds.format = dsp->strings[0].c_str();
      ds.name = dsp->strings[1].c_str();
      ds.flags = 2;
      ds.release = release_schema;
      ds.private_data = dsp;
    }
    for (auto& k : kp->kid_store) kp->kids.push_back(&k);
    for (auto& k : ksp->kid_store) ksp->kids.push_back(&k);
    memset(&ka, 0, sizeof(ka));
    ka.length = (int64_t)my_len;
    ka.offset = sliced && my_len ? (int64_t)off : 0;  // (no elements: no offset either -- consumers size the buffers by offset + length)
    ka.null_count = sliced ? (v.validity ? -1 : 0) : (int64_t)v.null_count;
    ka.n_buffers = (int64_t)kp->bufs.size();
    ka.buffers = kp->bufs.data();
    ka.n_children = (int64_t)kp->kids.size();
    ka.children = kp->kids.empty() ? nullptr : kp->kids.data();
    ka.dictionary = kp->dict_store.empty() ? nullptr : &kp->dict_store[0];
    ka.release = release_array;
    ka.private_data = kp;

    ksp->strings.reserve(2);
    ksp->strings.push_back(format);
    ksp->strings.push_back(name);  // owned by the schema
    memset(&ks, 0, sizeof(ks));
    ks.format = ksp->strings[0].c_str();
    ks.name = ksp->strings[1].c_str();
    // a root column is nullable when the batch has nulls (RecordBatch::try_from_iter, mod.rs:552-562); the fields of a Struct
    // and the elements of Lists come from the schema, where every field is nullable; so is a computed column, whatever the batch holds
    ks.flags = (v.null_count || co.parent >= 0 || sliced || co.computed) ? 2 /* ARROW_FLAG_NULLABLE */ : 0;
    ks.n_children = (int64_t)ksp->kids.size();
    ks.children = ksp->kids.empty() ? nullptr : ksp->kids.data();
    ks.dictionary = ksp->dict_store.empty() ? nullptr : &ksp->dict_store[0];
    ks.release = release_schema;
    ks.private_data = ksp;
  };
  std::vector<size_t> roots;
  for (size_t c = 0; c < nc; c++)
    if (r->cols[c].parent < 0) roots.push_back(c);
  ExportPriv* ap = new ExportPriv();
  SchemaPriv* sp = new SchemaPriv();
  ap->kid_store.resize(roots.size());
  sp->kid_store.resize(roots.size());
  sp->strings.reserve(2);
  for (size_t k = 0; k < roots.size(); k++) {
    const size_t c = roots[k];
    build(r, c, names && k < names->size() ? (*names)[k] : "c" + std::to_string(r->cols[c].column_id), false, 0, 0, ap->kid_store[k], sp->kid_store[k]);
    ap->kids.push_back(&ap->kid_store[k]);
    sp->kids.push_back(&sp->kid_store[k]);
  }
  memset(oa, 0, sizeof(*oa));
  ap->bufs.push_back(nullptr);
  oa->length = (int64_t)rows;
  oa->n_buffers = 1;
  oa->buffers = ap->bufs.data();
  oa->n_children = (int64_t)roots.size();
  oa->children = ap->kids.data();
  oa->release = release_array;
  oa->private_data = ap;
  memset(os, 0, sizeof(*os));
  sp->strings.push_back("+s");
  sp->strings.push_back("");
  os->format = sp->strings[sp->strings.size() - 2].c_str();
  os->name = sp->strings.back().c_str();
  os->n_children = (int64_t)roots.size();
  os->children = sp->kids.data();
  os->release = release_schema;
  os->private_data = sp;
  return ORCGPU_OK;
}

int orcgpu_result_export_batch(orcgpu_ctx* ctx, const orcgpu_result* r, uint32_t b, struct ArrowArray* oa, struct ArrowSchema* os) {
  return export_batch_named(ctx, r, b, oa, os, nullptr);
}

}  // extern "C"
