// writer_nested.hip -- the stripe writer's nested columns (orcgpu_writer.inc): Arrow's Struct / List / Map layout brought to the
// flat per-column form the encoders take.  ORC stores for each column one entry per existing row of its parent: a Struct's
// child has none where the Struct is null, a List's or Map's child holds the ranges of the non-null lists one behind the other.
//
// Per write and per Struct / List / Map column, from the column's own rows (NestRows + a map, its parent's work):
//   nest_kept_kernel    a presence byte per row; how many child rows each row keeps (Struct: 1 when valid; List: its length
//                       when valid), and the List's lengths; the offsets are the caller's, every pair is checked (`bad`)
//   enc_scan            the exclusive scan E of the kept counts: where each row's children start among the children's ORC rows
//   nest_desc_kernel    the children's rows: E's total many; one contiguous range of the child array when the total is the span
//                       from the first row's first child to the last row's last (nothing dropped in between): then no map
//   nest_fill_kernel    otherwise the map: for every child ORC row a search of its parent row in E, and its place in that range
//   nest_ends_kernel    the images of the slice ends (stripe cut): children before each end
// and for a leaf whose rows are a map, the gather of its validity bits, values, string offsets + bytes through the map
// (nest_gather_*), after which the leaf is an ordinary array of its ORC rows.
//
// A child's index q counts in the child array's logical rows before the array's own offset; maps hold q - lo (lo: the first
// index the host's two end offsets allow), 32 bits.  Once `bad` is set nothing downstream reads through an offset.

struct NestRows {
  uint64_t n, start;     // rows; contiguous: they are start .. start + n
  uint32_t contiguous, pad;
};

__device__ __forceinline__ uint64_t nest_q(const NestRows* r, const uint32_t* map, uint64_t lo, uint64_t i) {
  return r->contiguous ? r->start + i : lo + map[i];
}
__device__ __forceinline__ int64_t nest_off(const void* offsets, int offset_bytes, int64_t i) {
  return offset_bytes == 4 ? (int64_t)((const int32_t*)offsets)[i] : ((const int64_t*)offsets)[i];
}

// rows 0 .. cap: past rows->n zero.  validity: the copy's bit (q + vbit); offsets: the copy's entry (q + oadj); offset_bytes 0: Struct.
// A List's every pair of offsets lies in [kid_lo, kid_hi] (the host's two ends) and ascends, else `bad`.
extern "C" __global__ void __launch_bounds__(256) nest_kept_kernel(const NestRows* rows, const uint32_t* map, uint64_t lo, uint64_t cap, const uint8_t* validity,
                                                                   int64_t vbit, const void* offsets, int64_t oadj, int offset_bytes, int64_t kid_lo,
                                                                   int64_t kid_hi, uint8_t* pres, uint32_t* kept, void* lengths, const uint32_t* bad_in,
                                                                   uint32_t* bad) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cap) return;
  uint32_t k = 0, p = 0;
  int64_t len = 0;
  if (!*bad_in && i < rows->n) {
    const int64_t q = (int64_t)nest_q(rows, map, lo, i);
    p = 1;
    if (validity) {
      const int64_t b = q + vbit;
      p = (validity[b >> 3] >> (b & 7)) & 1;
    }
    if (offset_bytes) {
      const int64_t a = nest_off(offsets, offset_bytes, q + oadj), e = nest_off(offsets, offset_bytes, q + oadj + 1);
      if (a < kid_lo || e > kid_hi || e < a || e - a > 0x7fffffffll) *bad = 1;
      else len = e - a;
      k = p ? (uint32_t)len : 0u;
    } else {
      k = p;
    }
  }
  pres[i] = (uint8_t)p;
  kept[i] = k;
  if (offset_bytes == 4) ((int32_t*)lengths)[i] = (int32_t)len;
  else if (offset_bytes == 8) ((int64_t*)lengths)[i] = len;
}

// one thread: the children's rows from the scan's total
extern "C" __global__ void __launch_bounds__(64) nest_desc_kernel(const NestRows* rows, const uint32_t* map, uint64_t lo, const void* offsets, int64_t oadj,
                                                                  int offset_bytes, const uint64_t* total, uint64_t kid_cap, NestRows* kids, uint32_t* bad) {
  if (threadIdx.x || blockIdx.x) return;
  NestRows k{0, 0, 1, 0};
  const uint64_t T = *total, n = rows->n;
  if (!*bad && T > kid_cap) *bad = 1;  // (cannot be with ascending offsets)
  if (!*bad && n && T) {
    const int64_t first = (int64_t)nest_q(rows, map, lo, 0), last = (int64_t)nest_q(rows, map, lo, n - 1);
    uint64_t span;
    if (offset_bytes) {
      const int64_t a = nest_off(offsets, offset_bytes, first + oadj);
      k.start = (uint64_t)a;
      span = (uint64_t)(nest_off(offsets, offset_bytes, last + oadj + 1) - a);
    } else {
      k.start = (uint64_t)first;
      span = (uint64_t)(last + 1 - first);
    }
    k.n = T;
    k.contiguous = T == span;
  }
  *kids = k;
}

// the children's map (only when their rows are no contiguous range): child ORC row k belongs to the last row i with E[i] <= k
extern "C" __global__ void __launch_bounds__(256) nest_fill_kernel(const NestRows* rows, const uint32_t* map, uint64_t lo, const void* offsets, int64_t oadj,
                                                                   int offset_bytes, const uint64_t* E, const NestRows* kids, uint64_t kid_lo, uint64_t kid_cap,
                                                                   uint32_t* kmap, const uint32_t* bad) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= kid_cap || *bad || kids->contiguous || k >= kids->n) return;
  uint64_t a = 0, b = rows->n;  // the first row whose E exceeds k
  while (a < b) {
    const uint64_t mid = (a + b) >> 1;
    if (E[mid] <= k) a = mid + 1;
    else b = mid;
  }
  const uint64_t i = a - 1;
  const uint64_t q = nest_q(rows, map, lo, i);
  const uint64_t kq = offset_bytes ? (uint64_t)nest_off(offsets, offset_bytes, (int64_t)q + oadj) + (k - E[i]) : q;
  kmap[k] = (uint32_t)(kq - kid_lo);
}

// the root's slice ends: rows before the end of slice j
extern "C" __global__ void __launch_bounds__(256) nest_root_ends_kernel(uint64_t n_rows, uint64_t batch_size, uint64_t n_slices, uint64_t* ends) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_slices) return;
  ends[j] = (j + 1) * batch_size < n_rows ? (j + 1) * batch_size : n_rows;
}
// their images: the children before a column's slice ends
extern "C" __global__ void __launch_bounds__(256) nest_ends_kernel(const uint64_t* ends, const NestRows* rows, const uint64_t* E, const uint64_t* total, uint64_t n_slices,
                                                                   uint64_t* kends, const uint32_t* bad) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_slices) return;
  const uint64_t e = ends[j];
  kends[j] = *bad ? 0 : (e < rows->n ? E[e] : *total);
}

// wr_slice_counts_kernel with the slice ends given (a slice may hold no row of a child)
extern "C" __global__ void __launch_bounds__(256) nest_slice_counts_kernel(const uint8_t* validity, const uint64_t* word_off, const uint64_t* row_dst,
                                                                           const uint32_t* vlen, uint64_t n_rows, const uint64_t* ends, uint64_t n_slices,
                                                                           uint64_t* cum_valid, uint64_t* cum_bytes) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_slices) return;
  const uint64_t end = ends[j] < n_rows ? ends[j] : n_rows;
  if (!end) {
    cum_valid[j] = 0;
    cum_bytes[j] = 0;
    return;
  }
  const uint64_t last = end - 1, wi = last >> 6;
  uint64_t word = 0;
  const uint64_t nb = (n_rows + 7) / 8;
  for (uint32_t k = 0; k < 8; k++) word |= wi * 8 + k < nb ? (uint64_t)validity[wi * 8 + k] << (8 * k) : 0;
  const uint32_t keep = (uint32_t)(last & 63) + 1;
  if (keep < 64) word &= (1ull << keep) - 1;
  cum_valid[j] = word_off[wi] + (uint64_t)__builtin_popcountll(word);
  cum_bytes[j] = row_dst ? row_dst[last] + vlen[last] : 0;
}

// ---- the gather of a leaf through its map -----------------------------------------------------------------------------------
// bits: a byte of the output per thread; src's bit (map[k] + bit_adj); src == nullptr: all set
extern "C" __global__ void __launch_bounds__(256) nest_gather_bits_kernel(const uint32_t* map, uint64_t n, const uint8_t* src, int64_t bit_adj, uint8_t* dst) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (n + 7) / 8) return;
  uint32_t x = 0;
  for (uint32_t k = 0; k < 8; k++) {
    const uint64_t r = i * 8 + k;
    if (r >= n) break;
    uint32_t bit = 1;
    if (src) {
      const int64_t b = (int64_t)map[r] + bit_adj;
      bit = (src[b >> 3] >> (b & 7)) & 1;
    }
    x |= bit << k;
  }
  dst[i] = (uint8_t)x;
}

// fixed-width values: 16 bytes of the output per thread, stored as one; the map is monotone, so a wavefront's loads fall in few
// lines.  src: the copy's element map[k].  dst: 16-byte aligned, room for the last store's spare elements.
struct alignas(16) Nest16 {
  uint64_t a, b;
};
template <typename T>
__global__ void __launch_bounds__(256) nest_gather_kernel(const uint32_t* map, uint64_t n, const T* src, Nest16* dst) {
  constexpr uint32_t PER = 16 / sizeof(T);
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t k0 = t * PER;
  if (k0 >= n) return;
  union {
    T v[PER];
    Nest16 q;
  } u;
  u.q = Nest16{0, 0};
  bool whole = false;
  if constexpr (PER >= 4) {  // (the map four entries at a load)
    whole = k0 + PER <= n;
    if (whole) {
#pragma unroll
      for (uint32_t j = 0; j < PER; j += 4) {
        const uint4 m = *(const uint4*)(map + k0 + j);
        u.v[j] = src[m.x];
        u.v[j + 1] = src[m.y];
        u.v[j + 2] = src[m.z];
        u.v[j + 3] = src[m.w];
      }
    }
  }
  if (!whole) {
#pragma unroll
    for (uint32_t j = 0; j < PER; j++)
      if (k0 + j < n) u.v[j] = src[map[k0 + j]];
  }
  dst[t] = u.q;
}

// strings: the gathered rows' lengths (every pair of offsets in [s_lo, s_hi] and ascending, else `bad` and no bytes) ...
extern "C" __global__ void __launch_bounds__(256) nest_str_lengths_kernel(const uint32_t* map, uint64_t n, const void* offsets, int offset_bytes, int64_t s_lo,
                                                                          int64_t s_hi, uint32_t* len, uint32_t* bad) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int64_t a = nest_off(offsets, offset_bytes, map[k]), e = nest_off(offsets, offset_bytes, (int64_t)map[k] + 1);
  uint32_t l = 0;
  if (a < s_lo || e > s_hi || e < a || e - a > 0xffffffffll) *bad = 1;
  else l = (uint32_t)(e - a);
  len[k] = l;
}
// ... and, a wavefront per row, their bytes one behind the other with the offsets that say so (dst: exclusive scan of len).
// data: the byte offsets count from.  Never at or past `cap`.
extern "C" __global__ void __launch_bounds__(256) nest_str_copy_kernel(const uint32_t* map, uint64_t n, const void* offsets, int offset_bytes, const uint64_t* dst,
                                                                       const uint32_t* len, const uint8_t* data, uint8_t* out, uint64_t cap, void* new_offsets) {
  const uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (k >= n) return;
  const uint64_t d = dst[k], l = len[k];
  if (lane == 0) {
    if (offset_bytes == 4) ((int32_t*)new_offsets)[k] = (int32_t)d;
    else ((int64_t*)new_offsets)[k] = (int64_t)d;
    if (k == n - 1) {
      if (offset_bytes == 4) ((int32_t*)new_offsets)[n] = (int32_t)(d + l);
      else ((int64_t*)new_offsets)[n] = (int64_t)(d + l);
    }
  }
  if (!l) return;
  const int64_t lo = nest_off(offsets, offset_bytes, map[k]);
  for (uint64_t i = lane; i < l && d + i < cap; i += 64) out[d + i] = data[lo + (int64_t)i];
}
