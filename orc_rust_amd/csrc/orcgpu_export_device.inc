// orcgpu_export_device.inc -- device-resident batches: the Arrow C Device Data Interface export of a result, DLPack tensors over
// its buffers, and the bitmap unpacking that consumers without a bitmap type need (device/export_kernels.hip).
//
// The device twin of orcgpu_export.inc: the same struct array per batch, but its buffer pointers are the result's own HBM
// (orcgpu_result_batch_view) and nothing is copied.  What keeps that memory alive and unchanged is device_hold.h: every exported
// array, every child moved out of one and every DLPack tensor holds a reference on the result.

namespace {

// Frees a result for good (orcgpu_result_free once no export holds it)
void result_destroy(void* p) {
  orcgpu_result* r = static_cast<orcgpu_result*>(p);
  for (auto* sub : r->subs) orcgpu_result_free(sub);
  if (r->mirror) r->mirror->unref();
  if (r->dev_ready) (void)hipEventDestroy(r->dev_ready);
  for (auto& a : r->arena) a.release();
  for (auto& a : r->chars) a.release();
  r->sel_arena.release();
  r->filt_arena.release();
  r->filt_tmp.release();
  delete r;
}

// "The result is complete": an event on the decode stream behind everything enqueued on it so far -- where
// orcgpu_result_fetch_async records the gate of its copies.  The file reader calls it once the stripe's decode, selection and
// filter are enqueued; a result decoded by hand gets it at its first export.
int result_mark_ready(orcgpu_ctx* ctx, orcgpu_result* r) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!r->dev_ready) HIP_TRY(ctx, hipEventCreateWithFlags(&r->dev_ready, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventRecord(r->dev_ready, ctx->stream));
  r->dev_ready_recorded = true;
  return ORCGPU_OK;
}

// What a DLPack tensor needs to know of a column, kept by the exported array
struct DeviceColumn {
  uint64_t rows = 0;
  uint8_t code = 0, bits = 8;   // DLDataType of the values (strings: of the offsets)
  bool wide = false;            // 16-byte values: int64 [n, 2]
  bool is_string = false, is_bool = false;
  const void* validity = nullptr;
  const void* values = nullptr;   // strings: the bytes
  const void* offsets = nullptr;
  uint64_t values_bytes = 0;
  // a dictionary-output column: the stripe's dictionary (DLPack buffers 3 and 4)
  bool has_dict = false;
  const void* dict_offsets = nullptr;
  const void* dict_values = nullptr;
  uint64_t dict_len = 0, dict_bytes = 0;
};

// private_data of a child array: it may be moved out of its parent and then lives, and is released, on its own
struct DeviceChildPriv {
  orcgpu_hold::Hold* hold = nullptr;
  const void* bufs[3] = {nullptr, nullptr, nullptr};
  // a dictionary-output column: ArrowArray::dictionary, a Utf8 array over the stripe's entries.  It is part of the child, goes where
  // the child is moved and is released with it; the memory it views is the result's, which the child's own reference keeps
  bool has_dict = false;
  ArrowArray dict;
  const void* dict_bufs[3] = {nullptr, nullptr, nullptr};
};
void release_device_dictionary(ArrowArray* a) {
  if (a) a->release = nullptr;  // (nothing of its own: see DeviceChildPriv)
}
// ... and of the struct array
struct DeviceExportPriv {
  orcgpu_hold::Hold* hold = nullptr;
  hipEvent_t event = nullptr;    // ArrowDeviceArray::sync_event points here; the event is the result's, which `hold` keeps alive
  int device = 0;
  const void* bufs[1] = {nullptr};
  std::vector<ArrowArray> kid_store;
  std::vector<ArrowArray*> kids;
  std::vector<DeviceColumn> cols;
};

void release_device_child(ArrowArray* a) {
  if (!a || !a->release) return;
  DeviceChildPriv* p = static_cast<DeviceChildPriv*>(a->private_data);
  a->release = nullptr;
  if (p) {
    if (p->has_dict && p->dict.release) p->dict.release(&p->dict);
    orcgpu_hold::hold_release(p->hold);
    delete p;
  }
}
void release_device_array(ArrowArray* a) {
  if (!a || !a->release) return;
  DeviceExportPriv* p = static_cast<DeviceExportPriv*>(a->private_data);
  a->release = nullptr;
  if (p) {
    for (auto& k : p->kid_store)
      if (k.release) k.release(&k);  // (a child moved elsewhere has release == NULL here)
    orcgpu_hold::hold_release(p->hold);
    delete p;
  }
}

// The one refusal of this path: flat schemas only (the file reader checks its projection once, an export its result's columns)
int refuse_nested(orcgpu_ctx* ctx, const std::string& name, const char* kind) {
  set_err(ctx, "column '%s': a %s column has no device-resident export (flat schemas only); project it away or read it through the host path",
          name.c_str(), kind);
  return ORCGPU_UNSUPPORTED;
}

void dl_deleter(DLManagedTensor* t);
struct DlpackCtx {
  orcgpu_hold::Hold* hold = nullptr;
  int64_t shape[2] = {0, 0};
  DLManagedTensor tensor;
};
void dl_deleter(DLManagedTensor* t) {
  if (!t) return;
  DlpackCtx* c = static_cast<DlpackCtx*>(t->manager_ctx);
  orcgpu_hold::hold_release(c->hold);
  delete c;
}

}  // namespace

extern "C" {

static int export_batch_device_named(orcgpu_ctx* ctx, const orcgpu_result* rc_, uint32_t b, struct ArrowDeviceArray* out, struct ArrowSchema* os,
                                     const std::vector<std::string>* names) {
  orcgpu_result* r = const_cast<orcgpu_result*>(rc_);
  if (!ctx || !r || !out || !os || b >= r->n_batches) return ORCGPU_INVALID_ARGUMENT;
  if (r->status && b >= r->err_batch) {
    set_err(ctx, "batch %u is at or past the failing batch %u", b, r->err_batch);
    return r->status;
  }
  const size_t nc = r->cols.size();
  for (size_t c = 0; c < nc; c++) {
    const ColumnOut& co = r->cols[c];
    if (co.is_struct || co.is_union || co.is_list || co.parent >= 0) {
      // (a result of the file reader never gets here: its projection was refused before anything was read)
      size_t root = c;
      while (r->cols[root].parent >= 0) root = (size_t)r->cols[root].parent;
      const ColumnOut& rc = r->cols[root];
      return refuse_nested(ctx, "c" + std::to_string(rc.column_id), rc.is_struct ? "Struct" : (rc.is_union ? "Union" : (rc.is_map ? "Map" : "List")));
    }
  }
  r->was_exported = true;
  if (!r->dev_ready_recorded) {
    int rc = result_mark_ready(ctx, r);
    if (rc) return rc;
  }
  if (!r->hold) r->hold = orcgpu_hold::hold_new(r, result_destroy, nullptr);
  const uint64_t rows = batch_rows(r, b);
  DeviceExportPriv* ap = new DeviceExportPriv();
  SchemaPriv* sp = new SchemaPriv();
  ap->hold = r->hold;
  orcgpu_hold::hold_acquire(r->hold);
  ap->event = r->dev_ready;
  ap->device = ctx->device;
  ap->kid_store.resize(nc);
  ap->cols.resize(nc);
  sp->kid_store.resize(nc);
  for (size_t c = 0; c < nc; c++) {
    const ColumnOut& co = r->cols[c];
    orcgpu_batch_view v;
    orcgpu_result_batch_view(r, b, (uint32_t)c, &v);
    DeviceChildPriv* kp = new DeviceChildPriv();
    kp->hold = r->hold;
    orcgpu_hold::hold_acquire(r->hold);
    // (the host export's buffers, as device pointers: no validity buffer when the batch has no null)
    kp->bufs[0] = v.validity;
    int nb = 2;
    if (co.is_string) {
      kp->bufs[1] = v.offsets;
      kp->bufs[2] = v.values;
      nb = 3;
    } else {
      kp->bufs[1] = v.values;
    }
    ArrowArray& ka = ap->kid_store[c];
    memset(&ka, 0, sizeof(ka));
    ka.length = (int64_t)rows;
    ka.null_count = (int64_t)v.null_count;
    ka.n_buffers = nb;
    ka.buffers = kp->bufs;
    ka.release = release_device_child;
    ka.private_data = kp;
    ap->kids.push_back(&ka);
    orcgpu_dictionary_view dv;
    memset(&dv, 0, sizeof(dv));
    if (co.dict_out) {
      orcgpu_result_dictionary_view(r, (uint32_t)c, &dv);
      kp->has_dict = true;
      kp->dict_bufs[1] = dv.offsets;
      kp->dict_bufs[2] = dv.values;
      memset(&kp->dict, 0, sizeof(kp->dict));
      kp->dict.length = (int64_t)dv.length;
      kp->dict.n_buffers = 3;
      kp->dict.buffers = kp->dict_bufs;
      kp->dict.release = release_device_dictionary;
      ka.dictionary = &kp->dict;
    }

    DeviceColumn& dc = ap->cols[c];
    dc.rows = rows;
    dc.is_string = co.is_string;
    dc.is_bool = co.is_bool;
    dc.validity = v.validity;
    dc.values = v.values;
    dc.offsets = v.offsets;
    dc.values_bytes = v.values_bytes;
    dc.wide = co.width == 16;
    const bool is_float = co.orc_type == ORCGPU_T_FLOAT || co.orc_type == ORCGPU_T_DOUBLE;
    dc.code = co.is_string ? kDLInt : (co.is_bool ? kDLUInt : (is_float ? kDLFloat : kDLInt));
    dc.bits = co.is_string ? 32 : (co.is_bool ? 8 : (dc.wide ? 64 : (uint8_t)(co.width * 8)));
    dc.has_dict = co.dict_out;
    dc.dict_offsets = dv.offsets;
    dc.dict_values = dv.values;
    dc.dict_len = dv.length;
    dc.dict_bytes = dv.values_bytes;

    SchemaPriv* ksp = new SchemaPriv();
    ksp->strings.reserve(2);
    ksp->strings.push_back(arrow_format(co));
    ksp->strings.push_back(names && c < names->size() ? (*names)[c] : "c" + std::to_string(co.column_id));
    ArrowSchema& ks = sp->kid_store[c];
    memset(&ks, 0, sizeof(ks));
    ks.format = ksp->strings[0].c_str();
    ks.name = ksp->strings[1].c_str();
    ks.flags = (v.null_count || co.computed) ? 2 /* ARROW_FLAG_NULLABLE; a computed column: always */ : 0;
    if (co.dict_out) {
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
      ks.dictionary = &ksp->dict_store[0];
    }
    ks.release = release_schema;
    ks.private_data = ksp;
    sp->kids.push_back(&ks);
  }
  memset(out, 0, sizeof(*out));
  ArrowArray* oa = &out->array;
  oa->length = (int64_t)rows;
  oa->n_buffers = 1;
  oa->buffers = ap->bufs;
  oa->n_children = (int64_t)nc;
  oa->children = ap->kids.data();
  oa->release = release_device_array;
  oa->private_data = ap;
  out->device_id = ctx->device;
  out->device_type = ARROW_DEVICE_ROCM;
  out->sync_event = &ap->event;
  memset(os, 0, sizeof(*os));
  sp->strings.reserve(2);
  sp->strings.push_back("+s");
  sp->strings.push_back("");
  os->format = sp->strings[0].c_str();
  os->name = sp->strings[1].c_str();
  os->n_children = (int64_t)nc;
  os->children = sp->kids.data();
  os->release = release_schema;
  os->private_data = sp;
  return ORCGPU_OK;
}

int orcgpu_result_export_batch_device(orcgpu_ctx* ctx, const orcgpu_result* r, uint32_t b, struct ArrowDeviceArray* out, struct ArrowSchema* os) {
  return export_batch_device_named(ctx, r, b, out, os, nullptr);
}

uint64_t orcgpu_result_buffer_bytes(const orcgpu_result* r) {
  if (!r) return 0;
  uint64_t n = 0;
  if (r->filtered) n = r->filt_used;
  else {
    for (int l = 0; l < kMaxLanes; l++) n += r->arena_used[l] + r->chars_used[l];
    if (r->selected) n += r->sel_used;
  }
  for (auto* sub : r->subs) n += orcgpu_result_buffer_bytes(sub);
  return n;
}

int orcgpu_device_array_wait(const struct ArrowDeviceArray* array, void* hip_stream) {
  if (!array || !array->array.release) return ORCGPU_INVALID_ARGUMENT;
  if (!array->sync_event) return ORCGPU_OK;
  if (array->device_type != ARROW_DEVICE_ROCM) return ORCGPU_INVALID_ARGUMENT;
  hipEvent_t ev = *static_cast<hipEvent_t*>(array->sync_event);
  const hipError_t e = hip_stream ? hipStreamWaitEvent(static_cast<hipStream_t>(hip_stream), ev, 0) : hipEventSynchronize(ev);
  return e == hipSuccess ? ORCGPU_OK : ORCGPU_HIP_ERROR;
}

int orcgpu_device_array_dlpack(const struct ArrowDeviceArray* array, uint32_t column, int buffer, void** out_tensor) {
  if (out_tensor) *out_tensor = nullptr;
  // (only arrays of this library: the tensor's reference is on the result behind its private data)
  if (!array || !out_tensor || array->array.release != release_device_array || !array->array.private_data) return ORCGPU_INVALID_ARGUMENT;
  const DeviceExportPriv* p = static_cast<const DeviceExportPriv*>(array->array.private_data);
  if (column >= p->cols.size()) return ORCGPU_INVALID_ARGUMENT;
  const DeviceColumn& dc = p->cols[column];
  const void* data = nullptr;
  DLDataType dt{kDLUInt, 8, 1};
  int ndim = 1;
  int64_t shape[2] = {0, 0};
  if (buffer == 0) {
    data = dc.validity;
    shape[0] = (int64_t)((dc.rows + 7) / 8);
  } else if (buffer == 1 && dc.is_string) {
    data = dc.offsets;
    dt = DLDataType{kDLInt, 32, 1};
    shape[0] = (int64_t)dc.rows + 1;
  } else if (buffer == 1 && dc.is_bool) {
    data = dc.values;
    shape[0] = (int64_t)((dc.rows + 7) / 8);
  } else if (buffer == 1) {
    data = dc.values;
    dt = DLDataType{dc.code, dc.bits, 1};
    shape[0] = (int64_t)dc.rows;
    if (dc.wide) {
      ndim = 2;
      shape[1] = 2;
    }
  } else if (buffer == 2 && dc.is_string) {
    data = dc.values;
    shape[0] = (int64_t)dc.values_bytes;
  } else if (buffer == 3 && dc.has_dict) {
    data = dc.dict_offsets;
    dt = DLDataType{kDLInt, 32, 1};
    shape[0] = data ? (int64_t)dc.dict_len + 1 : 0;
  } else if (buffer == 4 && dc.has_dict) {
    data = dc.dict_values;
    shape[0] = (int64_t)dc.dict_bytes;
  } else {
    return ORCGPU_INVALID_ARGUMENT;
  }
  if (!data || !shape[0]) return ORCGPU_INVALID_ARGUMENT;
  DlpackCtx* c = new DlpackCtx();
  c->hold = p->hold;
  orcgpu_hold::hold_acquire(p->hold);
  c->shape[0] = shape[0];
  c->shape[1] = shape[1];
  memset(&c->tensor, 0, sizeof(c->tensor));
  c->tensor.dl_tensor.data = const_cast<void*>(data);
  c->tensor.dl_tensor.device = DLDevice{kDLROCM, (int32_t)p->device};
  c->tensor.dl_tensor.ndim = ndim;
  c->tensor.dl_tensor.dtype = dt;
  c->tensor.dl_tensor.shape = c->shape;
  c->tensor.dl_tensor.strides = nullptr;
  c->tensor.dl_tensor.byte_offset = 0;
  c->tensor.manager_ctx = c;
  c->tensor.deleter = dl_deleter;
  *out_tensor = &c->tensor;
  return ORCGPU_OK;
}

int orcgpu_unpack_bits(orcgpu_ctx* ctx, const void* d_bits, uint64_t n, uint8_t* d_bytes, void* hip_stream) {
  if (!ctx || (n && (!d_bits || !d_bytes)) || n > (1ull << 40)) return ORCGPU_INVALID_ARGUMENT;
  if (!n) return ORCGPU_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // pieces of 2^30 bits, so that a launch's thread count (a lane per 16 output bytes) stays far below what one grid holds; a
  // piece starts on a whole input byte and leaves the output's alignment as it is
  constexpr uint64_t kPiece = 1ull << 30;
  for (uint64_t at = 0; at < n; at += kPiece) {
    const uint64_t m = std::min<uint64_t>(kPiece, n - at);
    const uint8_t* in = static_cast<const uint8_t*>(d_bits) + at / 8;
    uint8_t* out = d_bytes + at;
    const uint32_t head = (uint32_t)std::min<uint64_t>(m, (16 - (reinterpret_cast<uintptr_t>(out) & 15)) & 15);
    const uint64_t n_chunks = (m - head) / 16;
    const uint64_t tail = m - head - n_chunks * 16;
    HIP_TRY(ctx, launch(unpack_bits_kernel, n_chunks + head + tail, false, kUnpackBlock, static_cast<hipStream_t>(hip_stream), in, m, out, head, n_chunks));
  }
  return ORCGPU_OK;
}

}  // extern "C"
