// orcgpu_writer_write.inc -- a record batch taken into the ArrowWriter (orcgpu_writer.inc), ArrowWriter::write: 0 the columns'
// arrays located, 1 the nested columns taken in, 2 the leaf columns taken in, then the stripe cut (WrCut), which extends the open
// stripe by the batch's slices and flushes (orcgpu_writer_flush.inc) where the reference would.
namespace {

// a column's array, and the rows it can hold by the host's look at its parent's two end offsets: the parent's index q of a row
// lies in [qlo, qhi) and the row's place in the array's buffers is q + base; a List's or Map's offsets' values [klo, khi)
struct WrArr {
  const ArrowArray* a = nullptr;
  uint64_t base = 0;
  int64_t qlo = 0, qhi = 0, klo = 0, khi = 0;
};
// the rows of a column's children in this write, as the device found them
struct HostRows {
  uint64_t n, start;
  bool contiguous;
};

// one write call: what its steps hand on
struct WrBatch {
  orcgpu_writer* w;
  const ArrowArray* batch;
  const std::vector<int64_t>& dev_ends;  // the device string columns' first and last offsets
  bool* rejected;
  uint64_t R, bs, n_slices;  // rows, rows of a slice, slices
  size_t nc;
  bool on_device;
  uint64_t *d_cv = nullptr, *d_cb = nullptr;  // [col][slice] valid values / bytes before each slice end (device)
  uint32_t* d_bad = nullptr;                  // the columns' "bad offsets" words, then their "timestamp without an encoding" words
  std::vector<char> present0;                 // the columns' `present` before the call
  std::vector<WrArr> A;
  std::vector<HostRows> hrows;   // [column + 1], 0: the root's children
  std::vector<uint64_t> hends;   // [column + 1][slice]: rows of the column's children before each slice end
  const uint64_t* d_kends = nullptr;  // ... on the device
  std::vector<uint64_t> cv, cb;  // d_cv, d_cb on the host
  int reject() {  // nothing of the batch was taken: the writer stays as it was
    for (size_t k = 0; k < nc; k++) w->cols[k].present = present0[k];
    *rejected = true;
    return ORCGPU_INVALID_ARGUMENT;
  }
};

// 0. every column's array, and the rows it can hold.  The root is a Struct whose rows are 0 .. R; a Struct's child has its
// parent's q, a List's or Map's the offsets' values [klo, khi)
int wr_locate_arrays(WrBatch& b) {
  orcgpu_writer* w = b.w;
  orcgpu_ctx* ctx = w->ctx;
  const ArrowArray* batch = b.batch;
  const uint64_t R = b.R;
  const int64_t row0 = batch->offset;
  std::vector<WrArr>& A = b.A;
  auto reject = [&b]() { return b.reject(); };
  for (size_t ci = 0; ci < b.nc; ci++) {
    const WrCol& c = w->cols[ci];
    WrArr& x = A[ci];
    int64_t shift = row0;
    x.qlo = 0;
    x.qhi = (int64_t)R;
    if (c.parent < 0) {
      x.a = batch->children[c.child];
    } else {
      const WrCol& pc = w->cols[(size_t)c.parent];
      const WrArr& px = A[(size_t)c.parent];
      const ArrowArray* pa = px.a;
      if (pc.orc_kind == ORCGPU_T_MAP) {  // (the Map's entries: a Struct without nulls of the key and the value)
        if (pa->n_children != 1 || !pa->children || !pa->children[0] || pa->children[0]->offset < 0 || pa->children[0]->length < px.khi) return reject();
        pa = pa->children[0];
      }
      if (pa->n_children <= c.child || !pa->children) return reject();
      x.a = pa->children[c.child];
      if (pc.stream_kind == WR_STRUCT) shift = (int64_t)px.base, x.qlo = px.qlo, x.qhi = px.qhi;
      else shift = pc.orc_kind == ORCGPU_T_MAP ? pa->offset : 0, x.qlo = px.klo, x.qhi = px.khi;
    }
    const ArrowArray* a = x.a;
    if (!wr_array_ok(c, a)) return reject();
    if (a->length < x.qhi + shift) {
      set_err(ctx, "writer: column %zu ('%s') has %lld rows, fewer than its parent's offsets address", ci, c.path.c_str(), (long long)a->length);
      return reject();
    }
    x.base = (uint64_t)(shift + a->offset);
    const uint64_t cap = (uint64_t)(x.qhi - x.qlo);
    if (c.stream_kind != WR_STRUCT && cap && (!a->buffers[1] || (c.is_string && !a->buffers[2]))) return reject();
    if (c.stream_kind == WR_LIST && cap) {
      const uint8_t* o = (const uint8_t*)a->buffers[1];
      const uint64_t p0 = (uint64_t)x.qlo + x.base, p1 = (uint64_t)x.qhi + x.base;
      x.klo = c.elem == 4 ? (int64_t)((const int32_t*)o)[p0] : ((const int64_t*)o)[p0];
      x.khi = c.elem == 4 ? (int64_t)((const int32_t*)o)[p1] : ((const int64_t*)o)[p1];
      if (x.klo < 0 || x.khi < x.klo || (uint64_t)(x.khi - x.klo) >= 0xffffffffull - 1024) {
        set_err(ctx, "writer: the offsets of column %zu ('%s') are not ascending (or address 2^32 - 1024 rows or more)", ci, c.path.c_str());
        return reject();
      }
    }
  }
  return ORCGPU_OK;
}

// 1. nested schemas: the Struct / List / Map columns, parents first, without a host wait -- their presence, lengths and counts
// per slice, and their children's rows (device/writer_nested.hip).  What comes back in one wait: NestRows per column (0: the
// root's children), `bad`, and every column's slice ends
int wr_nested_intake(WrBatch& b) {
  orcgpu_writer* w = b.w;
  orcgpu_ctx* ctx = w->ctx;
  hipStream_t st = ctx->stream;
  const size_t nc = b.nc;
  const uint64_t R = b.R, bs = b.bs, n_slices = b.n_slices;
  uint64_t *d_cv = b.d_cv, *d_cb = b.d_cb;
  const std::vector<WrArr>& A = b.A;
  std::vector<HostRows>& hrows = b.hrows;
  auto reject = [&b]() { return b.reject(); };
  Bump N;
  const uint64_t o_desc = N.take((nc + 1) * sizeof(NestRows)), o_nbad = N.take(8), o_kends = N.take((nc + 1) * n_slices * 8);
  if (!wr_ensure(w, w->nest, N.off + kAlign)) return ORCGPU_HIP_ERROR;
  NestRows* d_desc = (NestRows*)(w->nest.p + o_desc);
  uint32_t* d_nbad = (uint32_t*)(w->nest.p + o_nbad);
  uint64_t* kends = (uint64_t*)(w->nest.p + o_kends);
  b.d_kends = kends;
  const NestRows root{R, 0, 1, 0};
  WR_TRY(hipMemsetAsync(d_nbad, 0, 8, st));
  WR_TRY(hipMemcpyAsync(d_desc, &root, sizeof root, hipMemcpyHostToDevice, st));
  WR_TRY(launch(nest_root_ends_kernel, n_slices, false, 256, st, R, bs, n_slices, kends));
  for (size_t ci = 0; ci < nc; ci++) {
    WrCol& c = w->cols[ci];
    WrColDev& d = w->dev[ci];
    if (!c.is_nest()) continue;
    const WrArr& x = A[ci];
    const ArrowArray* a = x.a;
    const uint8_t* validity = (const uint8_t*)a->buffers[0];
    if (validity) c.present = true;
    const bool is_list = c.stream_kind == WR_LIST;
    const uint64_t cap = (uint64_t)(x.qhi - x.qlo), lo = (uint64_t)x.qlo;
    const uint64_t kid_lo = is_list ? (uint64_t)x.klo : lo, kid_cap = is_list ? (uint64_t)(x.khi - x.klo) : cap;
    const NestRows* d_rows = d_desc + (c.parent + 1);
    const uint32_t* d_map = c.parent < 0 ? nullptr : (const uint32_t*)w->dev[(size_t)c.parent].k_map.p;
    const uint64_t* d_ends = kends + (uint64_t)(c.parent + 1) * n_slices;
    // the bytes the rows can occupy, brought over: [validity bytes][offsets]
    const uint64_t P = lo + x.base, vlo = P / 8, vhi = (P + cap + 7) / 8;
    Bump I;
    const uint64_t o_v = I.take(validity && cap ? vhi - vlo : 0), o_x = I.take(is_list && cap ? (cap + 1) * (uint64_t)c.elem : 0);
    if (!wr_ensure(w, d.b_tmp, I.off + kAlign)) return ORCGPU_HIP_ERROR;
    if (validity && cap) WR_TRY(hipMemcpyAsync(d.b_tmp.p + o_v, validity + vlo, vhi - vlo, hipMemcpyHostToDevice, st));
    if (is_list && cap)
      WR_TRY(hipMemcpyAsync(d.b_tmp.p + o_x, (const uint8_t*)a->buffers[1] + P * (uint64_t)c.elem, (cap + 1) * (uint64_t)c.elem, hipMemcpyHostToDevice, st));
    const uint8_t* d_validity = validity && cap ? d.b_tmp.p + o_v : nullptr;
    const int64_t vbit = (int64_t)x.base - (int64_t)(8 * vlo), oadj = -(int64_t)lo;
    const void* d_offsets = d.b_tmp.p + o_x;
    Bump T;
    const uint64_t n_words = (cap + 63) / 64;
    const uint64_t o_bits = T.take(n_words * 8 + 8), o_wcnt = T.take(n_words * 4), o_woff = T.take(n_words * 8), o_sums = T.take((n_words / 2048 + 2) * 8),
                   o_tot = T.take(16), o_kept = T.take(cap * 4), o_E = T.take(cap * 8 + 8), o_sums2 = T.take((cap / 2048 + 2) * 8), o_tot2 = T.take(16),
                   o_len = T.take(cap * (uint64_t)c.elem);
    if (!wr_ensure(w, d.b_bits, T.off + kAlign) || !wr_ensure(w, d.b_pres, cap + kAlign) || !wr_ensure(w, d.b_vals, cap * (uint64_t)c.elem + kAlign) ||
        !wr_ensure(w, d.k_map, kid_cap * 4 + kAlign))
      return ORCGPU_HIP_ERROR;
    uint8_t* t = d.b_bits.p;
    uint8_t* bits = t + o_bits;
    uint64_t* woff = (uint64_t*)(t + o_woff);
    uint64_t* E = (uint64_t*)(t + o_E);
    uint64_t* tot2 = (uint64_t*)(t + o_tot2);
    const int ob = is_list ? c.elem : 0;
    WR_TRY(launch(nest_kept_kernel, cap, false, 256, st, d_rows, d_map, lo, cap, d_validity, vbit, d_offsets, oadj, ob, x.klo, x.khi, d.b_pres.p,
                  (uint32_t*)(t + o_kept), (void*)(t + o_len), (const uint32_t*)d_nbad, d_nbad));
    WR_TRY(launch(enc_bytes_to_bits_kernel, (cap + 7) / 8, false, 256, st, (const uint8_t*)d.b_pres.p, cap, bits));
    WR_TRY(launch(enc_valid_counts_kernel, n_words, false, 256, st, (const uint8_t*)bits, cap, (uint32_t*)(t + o_wcnt)));
    int rc = enc_scan(ctx, st, (const uint32_t*)(t + o_wcnt), n_words, (uint64_t*)(t + o_sums), (uint64_t*)(t + o_tot), woff);
    if (rc) return rc;
    if (is_list)  // LENGTH: the valid rows' lengths
      WR_TRY(launch(enc_gather_valid_kernel, cap, false, 256, st, (const uint8_t*)bits, cap, (const uint64_t*)woff, (const void*)(t + o_len), c.elem, (void*)d.b_vals.p));
    WR_TRY(launch(nest_slice_counts_kernel, n_slices, false, 256, st, (const uint8_t*)bits, (const uint64_t*)woff, (const uint64_t*)nullptr, (const uint32_t*)nullptr, cap,
                  d_ends, n_slices, d_cv + ci * n_slices, d_cb + ci * n_slices));
    // the children's rows
    WR_TRY(hipMemsetAsync(tot2, 0, 8, st));
    rc = enc_scan(ctx, st, (const uint32_t*)(t + o_kept), cap, (uint64_t*)(t + o_sums2), tot2, E);
    if (rc) return rc;
    WR_TRY(launch(nest_desc_kernel, (uint64_t)1, true, 64, st, d_rows, d_map, lo, d_offsets, oadj, ob, (const uint64_t*)tot2, kid_cap, d_desc + (ci + 1), d_nbad));
    WR_TRY(launch(nest_fill_kernel, kid_cap, false, 256, st, d_rows, d_map, lo, d_offsets, oadj, ob, (const uint64_t*)E, (const NestRows*)(d_desc + (ci + 1)), kid_lo,
                  kid_cap, (uint32_t*)d.k_map.p, (const uint32_t*)d_nbad));
    WR_TRY(launch(nest_ends_kernel, n_slices, false, 256, st, d_ends, d_rows, (const uint64_t*)E, (const uint64_t*)tot2, n_slices, kends + (ci + 1) * n_slices,
                  (const uint32_t*)d_nbad));
  }
  std::vector<uint8_t> back(N.off);
  WR_TRY(hipMemcpyAsync(back.data(), w->nest.p, N.off, hipMemcpyDeviceToHost, st));
  int rc = wr_sync(w);
  if (rc) return rc;
  uint32_t nbad;
  memcpy(&nbad, back.data() + o_nbad, 4);
  if (nbad) {
    set_err(ctx, "writer: the offsets of a List or Map column are not ascending, or address rows beyond its child");
    return reject();
  }
  const NestRows* hd = (const NestRows*)(back.data() + o_desc);
  for (size_t k = 1; k <= nc; k++)
    if (w->cols[k - 1].is_nest()) hrows[k] = HostRows{hd[k].n, hd[k].start, hd[k].contiguous != 0};
  b.hends.resize((nc + 1) * n_slices);
  memcpy(b.hends.data(), back.data() + o_kends, (nc + 1) * n_slices * 8);
  return ORCGPU_OK;
}

// a leaf column's rows of this write as the kernels read them
struct WrLeaf {
  uint64_t Rc = 0, off = 0, vb = 0;  // the column's rows in this write, the first one's place in its array, their validity bytes
  const uint8_t *validity = nullptr, *values = nullptr, *strdata = nullptr;  // the array's buffers
  // the input on the device: bits from `off`, values from `off`
  const uint8_t* d_valsrc = nullptr;  // validity bits, starting at bit d_valbit
  uint64_t d_valbit = 0;
  const uint8_t* d_values = nullptr;  // fixed width: values from row `off`; Boolean: bits (d_vbit); strings: offsets from row `off`
  uint64_t d_vbit = 0;
  const uint8_t* d_strbase = nullptr;  // strings: the byte the offsets count from
  uint64_t str_hi = 0;                 // strings: bytes addressed below offsets[off + Rc] (a bound of the valid rows' bytes)
};

// 2a. a leaf column in host memory: the bytes its rows occupy, brought over: [validity bytes][values / bits / offsets][string
// bytes] -- the slice's, or for the gather every row's the map can name: [qlo, qhi)
int wr_leaf_from_host(WrBatch& b, size_t ci, WrLeaf& L) {
  orcgpu_writer* w = b.w;
  orcgpu_ctx* ctx = w->ctx;
  hipStream_t st = ctx->stream;
  const WrCol& c = w->cols[ci];
  WrColDev& d = w->dev[ci];
  const WrArr& x = b.A[ci];
  const HostRows& hr = b.hrows[(size_t)(c.parent + 1)];
  uint32_t* d_bad = b.d_bad;
  auto reject = [&b]() { return b.reject(); };
  const uint64_t first = hr.contiguous ? L.off : (uint64_t)x.qlo + x.base, count = hr.contiguous ? L.Rc : (uint64_t)(x.qhi - x.qlo);
  const uint64_t vlo = first / 8, vhi = (first + count + 7) / 8;
  uint64_t val_lo = 0, val_n = 0;
  int64_t s_lo = 0, s_hi = 0;
  if (c.stream_kind == WR_BOOL) {
    val_lo = vlo;
    val_n = vhi - vlo;
  } else {
    val_lo = first * (uint64_t)c.elem;
    val_n = (count + (c.is_string ? 1 : 0)) * (uint64_t)c.elem;
  }
  if (c.is_string) {
    if (c.elem == 4) {
      s_lo = ((const int32_t*)L.values)[first];
      s_hi = ((const int32_t*)L.values)[first + count];
    } else {
      s_lo = ((const int64_t*)L.values)[first];
      s_hi = ((const int64_t*)L.values)[first + count];
    }
    if (s_lo < 0 || s_hi < s_lo) {
      set_err(ctx, "writer: the offsets of column %zu are not ascending", ci);
      return reject();
    }
    L.str_hi = (uint64_t)(s_hi - s_lo);
  }
  Bump I;
  const uint64_t o_v = I.take(L.validity ? vhi - vlo : 0), o_x = I.take(val_n), o_s = I.take(L.str_hi);
  if (!wr_ensure(w, d.b_tmp, I.off + kAlign)) return ORCGPU_HIP_ERROR;
  if (L.validity) WR_TRY(hipMemcpyAsync(d.b_tmp.p + o_v, L.validity + vlo, vhi - vlo, hipMemcpyHostToDevice, st));
  if (val_n) WR_TRY(hipMemcpyAsync(d.b_tmp.p + o_x, L.values + val_lo, val_n, hipMemcpyHostToDevice, st));
  if (L.str_hi) WR_TRY(hipMemcpyAsync(d.b_tmp.p + o_s, L.strdata + s_lo, L.str_hi, hipMemcpyHostToDevice, st));
  if (hr.contiguous) {
    L.d_valsrc = L.validity ? d.b_tmp.p + o_v : nullptr;
    L.d_valbit = L.off & 7;
    L.d_values = d.b_tmp.p + o_x;
    L.d_vbit = L.off & 7;
    L.d_strbase = d.b_tmp.p + o_s - s_lo;  // (addressed at offsets >= s_lo only)
  } else {
    // the gather: the column's ORC rows as an array of their own -- validity, values (Boolean: bits), offsets + bytes
    const uint32_t* d_map = (const uint32_t*)w->dev[(size_t)c.parent].k_map.p;  // q - qlo: the copies' row
    const int64_t bit_adj = (int64_t)(first - 8 * vlo);
    Bump Gt;
    const uint64_t o_gv = Gt.take(L.vb + 16), o_gx = Gt.take(c.stream_kind == WR_BOOL ? L.vb + 16 : (L.Rc + 1) * (uint64_t)c.elem + 16), o_gs = Gt.take(L.str_hi),
                   o_gl = Gt.take(c.is_string ? L.Rc * 4 : 0), o_gd = Gt.take(c.is_string ? L.Rc * 8 : 0), o_gsum = Gt.take((L.Rc / 2048 + 2) * 8), o_gtot = Gt.take(16);
    if (!wr_ensure(w, d.b_gath, Gt.off + kAlign)) return ORCGPU_HIP_ERROR;
    uint8_t* g = d.b_gath.p;
    if (L.validity) WR_TRY(launch(nest_gather_bits_kernel, L.vb, false, 256, st, d_map, L.Rc, (const uint8_t*)(d.b_tmp.p + o_v), bit_adj, g + o_gv));
    const uint8_t* src = d.b_tmp.p + o_x;
    const uint64_t n16 = (L.Rc * (uint64_t)c.elem + 15) / 16;
    if (c.stream_kind == WR_BOOL) {
      WR_TRY(launch(nest_gather_bits_kernel, L.vb, false, 256, st, d_map, L.Rc, src, bit_adj, g + o_gx));
    } else if (c.is_string) {
      WR_TRY(launch(nest_str_lengths_kernel, L.Rc, false, 256, st, d_map, L.Rc, (const void*)src, c.elem, (int64_t)s_lo, (int64_t)s_hi, (uint32_t*)(g + o_gl), d_bad + ci));
      int rc = enc_scan(ctx, st, (const uint32_t*)(g + o_gl), L.Rc, (uint64_t*)(g + o_gsum), (uint64_t*)(g + o_gtot), (uint64_t*)(g + o_gd));
      if (rc) return rc;
      WR_TRY(launch(nest_str_copy_kernel, (L.Rc + 3) / 4, true, 256, st, d_map, L.Rc, (const void*)src, c.elem, (const uint64_t*)(g + o_gd), (const uint32_t*)(g + o_gl),
                    (const uint8_t*)(d.b_tmp.p + o_s - s_lo), g + o_gs, L.str_hi, (void*)(g + o_gx)));
    } else if (c.elem == 1) {
      WR_TRY(launch(nest_gather_kernel<uint8_t>, n16, false, 256, st, d_map, L.Rc, (const uint8_t*)src, (Nest16*)(g + o_gx)));
    } else if (c.elem == 2) {
      WR_TRY(launch(nest_gather_kernel<uint16_t>, n16, false, 256, st, d_map, L.Rc, (const uint16_t*)src, (Nest16*)(g + o_gx)));
    } else if (c.elem == 4) {
      WR_TRY(launch(nest_gather_kernel<uint32_t>, n16, false, 256, st, d_map, L.Rc, (const uint32_t*)src, (Nest16*)(g + o_gx)));
    } else if (c.elem == 8) {
      WR_TRY(launch(nest_gather_kernel<uint64_t>, n16, false, 256, st, d_map, L.Rc, (const uint64_t*)src, (Nest16*)(g + o_gx)));
    } else {
      WR_TRY(launch(nest_gather_kernel<Nest16>, n16, false, 256, st, d_map, L.Rc, (const Nest16*)src, (Nest16*)(g + o_gx)));
    }
    L.d_valsrc = L.validity ? g + o_gv : nullptr;
    L.d_values = g + o_gx;
    L.d_strbase = g + o_gs;
  }
  return ORCGPU_OK;
}

// 2b. ... -> presence bytes, the valid rows' values, the strings' bytes; counts per slice
int wr_leaf_values(WrBatch& b, size_t ci, WrLeaf& L) {
  orcgpu_writer* w = b.w;
  orcgpu_ctx* ctx = w->ctx;
  hipStream_t st = ctx->stream;
  const WrCol& c = w->cols[ci];
  WrColDev& d = w->dev[ci];
  const size_t nc = b.nc;
  const uint64_t bs = b.bs, n_slices = b.n_slices;
  uint64_t *d_cv = b.d_cv, *d_cb = b.d_cb;
  uint32_t* d_bad = b.d_bad;
  const uint64_t* d_kends = b.d_kends;
  // presence: a bitmap from bit 0 (all set without a validity buffer) and its bytes
  Bump T;
  const uint64_t n_words = (L.Rc + 63) / 64;
  if (c.stream_kind == WR_DECIMAL) L.str_hi = L.Rc * (uint64_t)WR_DEC_MAX_BYTES;  // (the varints' bytes: a bound)
  const uint64_t o_bits = T.take(n_words * 8 + 8), o_vbits = T.take(c.stream_kind == WR_BOOL ? n_words * 8 + 8 : 0), o_wcnt = T.take(n_words * 4),
                 o_woff = T.take(n_words * 8), o_sums = T.take((n_words / 2048 + 2) * 8), o_tot = T.take(16),
                 o_len = T.take(c.is_string ? L.Rc * (uint64_t)c.elem : 0), o_vlen = T.take(c.has_bytes() ? L.Rc * 4 : 0),
                 o_dst = T.take(c.has_bytes() ? L.Rc * 8 : 0), o_sums2 = T.take((L.Rc / 2048 + 2) * 8), o_tot2 = T.take(16);
  if (!wr_ensure(w, d.b_bits, T.off + kAlign) || !wr_ensure(w, d.b_pres, L.Rc + kAlign) || !wr_ensure(w, d.b_vals, (c.stream_kind == WR_DECIMAL && !w->stride ? 0 : L.Rc * (uint64_t)c.elem) + kAlign) ||
      !wr_ensure(w, d.b_data, L.str_hi + kAlign) || !wr_ensure(w, d.b_vals2, (c.stream_kind == WR_TIMESTAMP ? L.Rc * 8 : 0) + kAlign))
    return ORCGPU_HIP_ERROR;
  uint8_t* t = d.b_bits.p;
  uint8_t* bits = t + o_bits;
  uint64_t* woff = (uint64_t*)(t + o_woff);
  WR_TRY(launch(wr_bits_kernel, L.vb, false, 256, st, L.d_valsrc, L.d_valbit, L.Rc, bits));
  WR_TRY(launch(wr_bits_to_bytes_kernel, L.Rc, false, 256, st, (const uint8_t*)bits, L.Rc, d.b_pres.p));
  WR_TRY(launch(enc_valid_counts_kernel, n_words, false, 256, st, (const uint8_t*)bits, L.Rc, (uint32_t*)(t + o_wcnt)));
  int rc = enc_scan(ctx, st, (const uint32_t*)(t + o_wcnt), n_words, (uint64_t*)(t + o_sums), (uint64_t*)(t + o_tot), woff);
  if (rc) return rc;
  const uint64_t* row_dst = nullptr;
  const uint32_t* vlen = nullptr;
  if (c.stream_kind == WR_BOOL) {  // the valid rows' Boolean values as 0 / 1 bytes
    WR_TRY(launch(wr_bits_kernel, L.vb, false, 256, st, (const uint8_t*)L.d_values, L.d_vbit, L.Rc, t + o_vbits));
    WR_TRY(launch(enc_gather_valid_kernel, L.Rc, false, 256, st, (const uint8_t*)bits, L.Rc, (const uint64_t*)woff, (const void*)(t + o_vbits), 0, (void*)d.b_vals.p));
  } else if (c.stream_kind == WR_TIMESTAMP) {  // the valid rows' seconds since 2015 and nanosecond codes
    WR_TRY(launch(wr_timestamp_kernel, L.Rc, false, 256, st, (const uint8_t*)bits, L.Rc, (const uint64_t*)woff, (const int64_t*)L.d_values, c.ups, c.npu,
                  (int64_t*)d.b_vals.p, (uint64_t*)d.b_vals2.p, d_bad + nc + ci));
  } else if (c.stream_kind == WR_DECIMAL) {  // the valid rows' varints one behind the other, and the values themselves (statistics)
    WR_TRY(launch(wr_dec_lengths_kernel, L.Rc, false, 256, st, (const uint64_t*)L.d_values, (const uint8_t*)bits, L.Rc, (uint32_t*)(t + o_vlen)));
    rc = enc_scan(ctx, st, (const uint32_t*)(t + o_vlen), L.Rc, (uint64_t*)(t + o_sums2), (uint64_t*)(t + o_tot2), (uint64_t*)(t + o_dst));
    if (rc) return rc;
    WR_TRY(launch(wr_dec_pack_kernel, (L.Rc + 255) / 256, true, 256, st, (const uint64_t*)L.d_values, (const uint8_t*)bits, L.Rc, (const uint64_t*)(t + o_dst),
                  (const uint32_t*)(t + o_vlen), d.b_data.p, L.str_hi));
    if (w->stride)  // (the values themselves: only the row index statistics read them)
      WR_TRY(launch(enc_gather_valid_kernel, L.Rc, false, 256, st, (const uint8_t*)bits, L.Rc, (const uint64_t*)woff, (const void*)L.d_values, 16, (void*)d.b_vals.p));
    row_dst = (const uint64_t*)(t + o_dst);
    vlen = (const uint32_t*)(t + o_vlen);
  } else if (!c.is_string) {
    WR_TRY(launch(enc_gather_valid_kernel, L.Rc, false, 256, st, (const uint8_t*)bits, L.Rc, (const uint64_t*)woff, (const void*)L.d_values, c.elem, (void*)d.b_vals.p));
  } else {
    WR_TRY(launch(enc_lengths_kernel, L.Rc, false, 256, st, (const void*)L.d_values, c.elem, (const uint8_t*)bits, L.Rc, (void*)(t + o_len), (uint32_t*)(t + o_vlen),
                  d_bad + ci));
    rc = enc_scan(ctx, st, (const uint32_t*)(t + o_vlen), L.Rc, (uint64_t*)(t + o_sums2), (uint64_t*)(t + o_tot2), (uint64_t*)(t + o_dst));
    if (rc) return rc;
    // (bounded by str_hi: the offsets are checked when the counts come back, `bad`)
    WR_TRY(launch(wr_copy_strings_kernel, (L.Rc + 3) / 4, true, 256, st, (const uint8_t*)bits, (const void*)L.d_values, c.elem, L.Rc, (const uint64_t*)(t + o_dst),
                  L.d_strbase, d.b_data.p, L.str_hi));
    WR_TRY(launch(enc_gather_valid_kernel, L.Rc, false, 256, st, (const uint8_t*)bits, L.Rc, (const uint64_t*)woff, (const void*)(t + o_len), c.elem, (void*)d.b_vals.p));
    row_dst = (const uint64_t*)(t + o_dst);
    vlen = (const uint32_t*)(t + o_vlen);
  }
  if (w->nested)
    WR_TRY(launch(nest_slice_counts_kernel, n_slices, false, 256, st, (const uint8_t*)bits, (const uint64_t*)woff, row_dst, vlen, L.Rc,
                  d_kends + (uint64_t)(c.parent + 1) * n_slices, n_slices, d_cv + ci * n_slices, d_cb + ci * n_slices));
  else
    WR_TRY(launch(wr_slice_counts_kernel, n_slices, false, 256, st, (const uint8_t*)bits, (const uint64_t*)woff, row_dst, vlen, L.Rc, bs, n_slices, d_cv + ci * n_slices,
                  d_cb + ci * n_slices));
  return ORCGPU_OK;
}

// 2. a leaf column of the batch.  Its rows are a slice of its array (below the root always; below a Struct / List when nothing
// was dropped), or gathered through the map
int wr_leaf_intake(WrBatch& b, size_t ci) {
  orcgpu_writer* w = b.w;
  orcgpu_ctx* ctx = w->ctx;
  hipStream_t st = ctx->stream;
  WrCol& c = w->cols[ci];
  const WrArr& x = b.A[ci];
  const ArrowArray* a = x.a;
  const HostRows& hr = b.hrows[(size_t)(c.parent + 1)];
  WrLeaf L;
  L.Rc = hr.n;
  L.validity = (const uint8_t*)a->buffers[0];
  L.values = (const uint8_t*)a->buffers[1];
  L.strdata = c.is_string ? (const uint8_t*)a->buffers[2] : nullptr;
  if (L.validity) c.present = true;
  if (!L.Rc) {
    WR_TRY(hipMemsetAsync(b.d_cv + ci * b.n_slices, 0, b.n_slices * 8, st));
    WR_TRY(hipMemsetAsync(b.d_cb + ci * b.n_slices, 0, b.n_slices * 8, st));
    return ORCGPU_OK;
  }
  if (!L.values || (c.is_string && !L.strdata)) return ORCGPU_INVALID_ARGUMENT;
  if (c.parent >= 0) (hr.contiguous ? w->nested_slices : w->nested_gathers)++;
  L.off = hr.start + x.base;
  L.vb = (L.Rc + 7) / 8;
  if (b.on_device) {
    L.d_valsrc = L.validity;
    L.d_valbit = L.off;
    if (c.stream_kind == WR_BOOL) {
      L.d_values = L.values;
      L.d_vbit = L.off;
    } else {
      L.d_values = L.values + L.off * (uint64_t)c.elem;
    }
    if (c.is_string) {  // (read and checked by orcgpu_writer_write before anything changed)
      L.d_strbase = L.strdata;
      L.str_hi = (uint64_t)(b.dev_ends[2 * ci + 1] - b.dev_ends[2 * ci]);
    }
  } else {
    const int rc = wr_leaf_from_host(b, ci, L);
    if (rc) return rc;
  }
  return wr_leaf_values(b, ci, L);
}

// the counts per slice and the columns' `bad` words, brought back in one wait
int wr_counts_back(WrBatch& b) {
  orcgpu_writer* w = b.w;
  orcgpu_ctx* ctx = w->ctx;
  hipStream_t st = ctx->stream;
  const size_t nc = b.nc;
  const uint64_t n_slices = b.n_slices;
  b.cv.assign(nc * n_slices, 0);
  b.cb.assign(nc * n_slices, 0);
  std::vector<uint32_t> bad(2 * nc);
  if (nc) {
    WR_TRY(hipMemcpyAsync(b.cv.data(), b.d_cv, nc * n_slices * 8, hipMemcpyDeviceToHost, st));
    WR_TRY(hipMemcpyAsync(b.cb.data(), b.d_cb, nc * n_slices * 8, hipMemcpyDeviceToHost, st));
    WR_TRY(hipMemcpyAsync(bad.data(), b.d_bad, nc * 8, hipMemcpyDeviceToHost, st));
  }
  int rc = wr_sync(w);
  if (rc) return rc;
  for (size_t ci = 0; ci < nc; ci++)
    if (bad[ci]) {
      set_err(ctx, "writer: the offsets of column %zu are not ascending (or a value is 4 GiB or longer)", ci);
      return w->nested ? b.reject() : ORCGPU_INVALID_ARGUMENT;
    }
  for (size_t ci = 0; ci < nc; ci++)
    if (bad[nc + ci]) {  // nothing of the batch was taken: the writer stays as it was
      set_err(ctx, "writer: column %zu holds a timestamp ORC cannot encode (within the second before 1970-01-01 00:00:00 but not on it, or its second too far from 2015 for i64)", ci);
      return b.reject();
    }
  return ORCGPU_OK;
}

// The stripe cut (arrow_writer.rs:103-124) over the batch's slices: slices that cannot reach the limit by an upper bound of the
// encoders' output are taken as they are; past them windows of the run analysis, growing geometrically.
struct WrCut {
  WrBatch& b;
  orcgpu_writer* w;
  std::vector<uint64_t> est;  // the run-length encoded terms after the analysed slices

  uint64_t V(size_t ci, uint64_t j) const { return j ? b.cv[ci * b.n_slices + j - 1] : 0; }  // valid rows before slice j
  uint64_t B(size_t ci, uint64_t j) const { return j ? b.cb[ci * b.n_slices + j - 1] : 0; }  // ... their bytes
  uint64_t rows_to(uint64_t j) const { return std::min<uint64_t>(j * b.bs, b.R); }           // rows before slice j
  // ... and a column's own rows before it: its parent's children's
  uint64_t RT(size_t ci, uint64_t j) const {
    if (!w->nested) return rows_to(j);
    return j ? b.hends[(size_t)(w->cols[ci].parent + 1) * b.n_slices + j - 1] : 0;
  }
  // a column's counts after the batch's slices [j0, j1) were added to the open stripe
  WrCounts counts(size_t ci, uint64_t j0, uint64_t j1) const {
    const WrCol& c = w->cols[ci];
    return WrCounts{c.rows + RT(ci, j1) - RT(ci, j0), c.n_valid + V(ci, j1) - V(ci, j0), c.n_bytes + B(ci, j1) - B(ci, j0)};
  }

  // the stripe's buffers extended by the batch's slices [j0, j1) (the counters move only with `commit`)
  int extend(uint64_t j0, uint64_t j1, bool commit) {
    orcgpu_ctx* ctx = w->ctx;
    hipStream_t st = ctx->stream;
    for (size_t ci = 0; ci < b.nc; ci++) {
      WrCol& c = w->cols[ci];
      WrColDev& d = w->dev[ci];
      const uint64_t dv = V(ci, j1) - V(ci, j0), dr = RT(ci, j1) - RT(ci, j0), db = B(ci, j1) - B(ci, j0);
      const uint64_t velem = c.stream_kind == WR_DECIMAL && !w->stride ? 0 : (uint64_t)c.elem;  // (Decimal128 values: kept for the row index only)
      const uint64_t nv = c.n_valid * velem, add = dv * velem;
      if (velem && !wr_reserve(w, d.vals, nv + add + kAlign, nv)) return ORCGPU_HIP_ERROR;
      if (add) WR_TRY(hipMemcpyAsync(d.vals.p + nv, d.b_vals.p + V(ci, j0) * velem, add, hipMemcpyDeviceToDevice, st));
      if (c.stream_kind == WR_TIMESTAMP || c.stream_kind == WR_DECIMAL) {
        const uint64_t e2 = (uint64_t)c.elem2(), nv2 = c.n_valid * e2;
        if (!wr_reserve(w, d.vals2, nv2 + dv * e2 + kAlign, nv2)) return ORCGPU_HIP_ERROR;
        if (dv && c.stream_kind == WR_TIMESTAMP) WR_TRY(hipMemcpyAsync(d.vals2.p + nv2, d.b_vals2.p + V(ci, j0) * e2, dv * e2, hipMemcpyDeviceToDevice, st));
        if (dv && c.stream_kind == WR_DECIMAL) WR_TRY(launch(wr_fill16_kernel, dv, false, 256, st, (uint16_t*)(d.vals2.p + nv2), dv, (uint16_t)c.scale));
      }
      if (commit) {
        if (!wr_reserve(w, d.pres, c.rows + dr + kAlign, c.rows)) return ORCGPU_HIP_ERROR;
        if (dr) WR_TRY(hipMemcpyAsync(d.pres.p + c.rows, d.b_pres.p + RT(ci, j0), dr, hipMemcpyDeviceToDevice, st));
        if (c.has_bytes()) {
          if (!wr_reserve(w, d.data, c.n_bytes + db + kAlign, c.n_bytes)) return ORCGPU_HIP_ERROR;
          if (db) WR_TRY(hipMemcpyAsync(d.data.p + c.n_bytes, d.b_data.p + B(ci, j0), db, hipMemcpyDeviceToDevice, st));
        }
        c.rows += dr;
        c.n_valid += dv;
        c.n_bytes += db;
      }
    }
    if (commit) w->rows += rows_to(j1) - rows_to(j0);
    return ORCGPU_OK;
  }

  // the summed estimate after slice j (j0 <= j) of the streams that are counted: floats, Booleans, string bytes, PRESENT; the
  // run-length encoded streams: exactly base_rle when the columns had base_valid values; each run written out since covers
  // values from then on, or from the run open then -- at most 512 values before: *rle_bound
  uint64_t counted(uint64_t j0, uint64_t j, uint64_t* rle_bound) const {
    uint64_t e = 0, bound = 0;
    for (size_t ci = 0; ci < b.nc; ci++) {
      const WrCol& c = w->cols[ci];
      WrStream s[WR_MAX_STREAMS];
      const int ns = wr_streams(c, counts(ci, j0, j + 1), false, s);
      for (int k = 0; k < ns; k++) {
        e += wr_counted(s[k]);
        bound += wr_runs_bound(s[k], s[k].n - c.base_valid + 512);
      }
    }
    if (rle_bound) *rle_bound = w->base_rle + bound;
    return e;
  }

  // the first slice in [j0, j1) after which the estimate exceeds the limit, or j1; -1: a device call failed.  The streams that go
  // through an encoder are planned over the stripe's values with the window's: Timestamp both (as two Int64 columns would
  // count), Decimal128 the scale alone (its DATA bytes are counted), every other column its one
  int64_t analyse(uint64_t j0, uint64_t j1) {
    orcgpu_ctx* ctx = w->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t win = j1 - j0;
    if (!wr_ensure(w, w->est, win * 8 + kAlign)) return -1;
    uint64_t* d_est = (uint64_t*)w->est.p;
    if (hipMemsetAsync(d_est, 0, win * 8, st) != hipSuccess) return -1;
    if (extend(j0, j1, false)) return -1;
    for (size_t ci = 0; ci < b.nc; ci++) {
      const WrCol& c = w->cols[ci];
      WrStream sd[WR_MAX_STREAMS];
      const int ns = wr_streams(c, counts(ci, j0, j1), false, sd);
      for (int k = 0; k < ns; k++) {
        if (sd[k].cost != WR_COST_RUNS) continue;
        EncJob J;
        J.kind = sd[k].enc == WR_ENC_BYTE_RLE ? 1 : 0;
        J.int_bytes = sd[k].width;
        J.is_signed = sd[k].is_signed;
        J.n = sd[k].n;
        J.values = w->dev[ci].src(sd[k].src);
        J.deferred = true;  // (no host wait: the run count stays on the device, the grids cover n runs)
        J.syncs = &w->round_trips;
        if (!J.n) continue;
        if (!wr_ensure(w, w->trig, J.n * 8 + kAlign)) return -1;  // (before the plan: growing waits, and the tables are the plan's)
        if (enc_plan(ctx, J)) return -1;
        uint64_t* d_trig = (uint64_t*)w->trig.p;
        hipError_t e = sd[k].enc == WR_ENC_RLE2 ? launch(wr_triggers_kernel<0>, (uint64_t)J.n_runs, false, 256, st, (const void*)J.values, J.int_bytes, (const uint32_t*)J.runs,
                                            J.d_n_runs, J.n, d_trig)
                                   : launch(wr_triggers_kernel<1>, (uint64_t)J.n_runs, false, 256, st, (const void*)J.values, 1, (const uint32_t*)J.runs, J.d_n_runs,
                                            J.n, d_trig);
        if (e != hipSuccess) return -1;
        // values after slice j: c.n_valid + cv[j] - V(j0)
        e = launch(wr_estimate_kernel, win, false, 256, st, (const uint64_t*)d_trig, (const uint32_t*)J.runs, (const uint32_t*)J.run_bytes, (const uint64_t*)J.offsets,
                   J.d_n_runs, J.kind, (const uint64_t*)(b.d_cv + ci * b.n_slices + j0), (int64_t)c.n_valid - (int64_t)V(ci, j0), win, d_est);
        if (e != hipSuccess) return -1;
      }
    }
    est.assign(win, 0);
    if (hipMemcpyAsync(est.data(), d_est, win * 8, hipMemcpyDeviceToHost, st) != hipSuccess || wr_sync(w)) return -1;
    for (uint64_t j = j0; j < j1; j++)
      if (est[j - j0] + counted(j0, j, nullptr) > w->stripe_byte_size) return (int64_t)j;
    return (int64_t)j1;
  }

  int run() {
    orcgpu_ctx* ctx = w->ctx;
    const uint64_t n_slices = b.n_slices;
    int rc;
    uint64_t j0 = 0;
    while (j0 < n_slices) {
      // slices that cannot reach the limit by the bound: taken as they are
      uint64_t js = j0;
      while (js < n_slices) {
        uint64_t bound;
        const uint64_t e = counted(j0, js, &bound);
        if (e + bound > w->stripe_byte_size) break;
        js++;
      }
      if (js == n_slices) {
        rc = extend(j0, n_slices, true);
        if (rc) return rc;
        break;
      }
      // the rest: windows of the run analysis, growing
      uint64_t win = std::max<uint64_t>(w->window_hint, js - j0 + 1);
      int64_t cut;
      for (;;) {
        const uint64_t j1 = std::min<uint64_t>(n_slices, j0 + win);
        cut = analyse(j0, j1);
        if (cut < 0) {
          if (ctx->err.empty()) set_err(ctx, "writer: the stripe analysis failed");
          return ORCGPU_HIP_ERROR;
        }
        if ((uint64_t)cut < j1 || j1 == n_slices) break;
        win *= 2;
      }
      if ((uint64_t)cut == n_slices) {
        rc = extend(j0, n_slices, true);
        if (rc) return rc;
        w->base_rle = est.back();  // (exact at the end of this write: later bounds start from it)
        for (auto& c : w->cols) c.base_valid = c.n_valid;
        break;
      }
      rc = extend(j0, (uint64_t)cut + 1, true);
      if (rc) return rc;
      rc = wr_flush(w);
      if (rc) return rc;
      w->window_hint = std::max<uint64_t>(1, (uint64_t)cut + 1 - j0);
      j0 = (uint64_t)cut + 1;
    }
    return ORCGPU_OK;
  }
};

// ArrowWriter::write after orcgpu_writer_write's checks; dev_ends: the device string columns' first and last offsets.
// *rejected: the batch holds a value without an encoding (INVALID_ARGUMENT) and the writer is as it was before the call
int wr_write(orcgpu_writer* w, const struct ArrowArray* batch, uint32_t flags, const std::vector<int64_t>& dev_ends, bool* rejected) {
  orcgpu_ctx* ctx = w->ctx;
  const uint64_t R = batch->length < 0 ? 0 : (uint64_t)batch->length;
  if (batch->n_children != (int64_t)w->root_kids.size() || (w->root_kids.size() && !batch->children)) return ORCGPU_INVALID_ARGUMENT;
  if (R == 0) return ORCGPU_OK;  // (no slice: step_by over an empty range)
  if (R >= 0xffffffffull - 1024) {
    set_err(ctx, "writer: %llu rows in one batch (fewer than 2^32 - 1024 per write)", (unsigned long long)R);
    return ORCGPU_INVALID_ARGUMENT;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t nc = w->cols.size();
  WrBatch b{w, batch, dev_ends, rejected, R, w->batch_size, (R + w->batch_size - 1) / w->batch_size, nc, (flags & ORCGPU_ENC_ON_DEVICE) != 0};
  const uint64_t n_slices = b.n_slices;
  if (!wr_ensure(w, w->slice_counts, nc * n_slices * 16 + 16 * nc + kAlign)) return ORCGPU_HIP_ERROR;
  b.d_cv = (uint64_t*)w->slice_counts.p;
  b.d_cb = b.d_cv + nc * n_slices;
  b.d_bad = (uint32_t*)(b.d_cb + nc * n_slices);
  if (nc) WR_TRY(hipMemsetAsync(b.d_bad, 0, nc * 8, ctx->stream));
  b.present0.resize(nc);
  for (size_t ci = 0; ci < nc; ci++) b.present0[ci] = w->cols[ci].present;
  b.A.resize(nc);
  b.hrows.assign(nc + 1, HostRows{R, 0, true});
  int rc = wr_locate_arrays(b);
  if (!rc && w->nested) rc = wr_nested_intake(b);
  for (size_t ci = 0; !rc && ci < nc; ci++)
    if (!w->cols[ci].is_nest()) rc = wr_leaf_intake(b, ci);
  if (!rc) rc = wr_counts_back(b);
  if (rc) return rc;
  WrCut cut{b, w, {}};
  rc = cut.run();
  return rc ? rc : wr_sync(w);  // (the caller may release the batch now)
}

}  // namespace
