// device/col_stats.hip -- the writer's row index (orcgpu_writer_set_row_index): the ColumnStatistics of every row group of every
// column of a stripe, and where each group starts in each stream.  Everything works on the stripe's device-resident form
// (orcgpu_writer.inc, WrCol / WrColDev): a presence byte per row, the valid values (Boolean: 0 / 1 bytes; strings: their lengths), the
// strings' bytes.  A job is one (column, row group): job j = column * G + group, G groups of `stride` rows in every column.
//
//   ix_count_kernel      valid values per job (a block per job, over the presence bytes)
//   ix_scan_kernel       exclusive scan of a u64 array (one block): the jobs' first values, first string bytes, side offsets
//   ix_bytes_kernel      string bytes per job
//   ix_stats_kernel      the job's record (a block per job): count, has_null, min / max, 128-bit integer sum, double-double sum,
//                        true count, string bytes; string min / max by an 8-byte big-endian key, full compares on ties
//   ix_side_kernel       the string minimum's and maximum's first IX_STR_KEEP bytes into the side buffer
//   ix_pos_kernel        a lane per group of one stream: its entry position, by a binary search of the encoder's run table
//   ix_map_kernel        compressed files: uncompressed offsets -> (chunk header in the compressed stream, bytes into the chunk)

#include "writer_kinds.h"  // WrKind, IX_STR_KEEP, IxRec

#define IX_COLS_PER_ARG 16

struct IxCol {
  const uint8_t* pres;  // a byte per row of the stripe
  const void* vals;     // the valid values in `elem` bytes each
  const uint8_t* data;  // strings' bytes (Timestamp: the nanosecond codes, vals the stored seconds)
  int32_t kind;         // WrKind
  int32_t elem;
  int32_t minmax;       // strings: 1 with a minimum / maximum (Utf8), 0 without (Binary)
  int32_t pad;
};
struct IxColArgs {
  uint32_t at, n;
  IxCol c[IX_COLS_PER_ARG];
};

__global__ __launch_bounds__(64) void ix_put_cols_kernel(IxColArgs a, IxCol* dst) {
  if (threadIdx.x < a.n) dst[a.at + threadIdx.x] = a.c[threadIdx.x];
}

__device__ __forceinline__ uint64_t ix_block_sum(uint64_t v, uint64_t* lds) {
  const uint32_t t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (uint32_t d = 128; d > 0; d >>= 1) {
    if (t < d) lds[t] += lds[t + d];
    __syncthreads();
  }
  const uint64_t s = lds[0];
  __syncthreads();
  return s;
}

__device__ __forceinline__ uint64_t ix_len(const void* vals, int elem, uint64_t i) {
  return elem == 4 ? (uint64_t)((const uint32_t*)vals)[i] : ((const uint64_t*)vals)[i];
}

extern "C" __global__ void __launch_bounds__(256) ix_count_kernel(const IxCol* cols, uint64_t rows, uint64_t S, uint64_t G, uint64_t* cnt) {
  __shared__ uint64_t lds[256];
  const uint64_t j = blockIdx.x, c = j / G, g = j % G;
  const uint64_t r0 = g * S, r1 = min(r0 + S, rows);
  const uint8_t* p = cols[c].pres;
  uint64_t n = 0;
  for (uint64_t r = r0 + threadIdx.x; r < r1; r += 256) n += p[r];
  n = ix_block_sum(n, lds);
  if (threadIdx.x == 0) cnt[j] = n;
}

// out[i] = in[0] + .. + in[i-1], out[n] = the total
extern "C" __global__ void __launch_bounds__(1024) ix_scan_kernel(const uint64_t* in, uint64_t n, uint64_t* out) {
  __shared__ uint64_t s[1024];
  __shared__ uint64_t carry;
  const uint32_t t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (uint64_t i0 = 0; i0 < n; i0 += 1024) {
    const uint64_t i = i0 + t;
    const uint64_t v = i < n ? in[i] : 0;
    s[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d *= 2) {
      const uint64_t a = t >= d ? s[t - d] : 0;
      __syncthreads();
      s[t] += a;
      __syncthreads();
    }
    if (i < n) out[i] = carry + s[t] - v;
    __syncthreads();
    if (t == 1023) carry += s[1023];
    __syncthreads();
  }
  if (t == 0) out[n] = carry;
}

extern "C" __global__ void __launch_bounds__(256) ix_bytes_kernel(const IxCol* cols, uint64_t G, const uint64_t* cnt, const uint64_t* vscan, uint64_t* blen) {
  __shared__ uint64_t lds[256];
  const uint64_t j = blockIdx.x, c = j / G;
  const IxCol col = cols[c];
  if (col.kind != WR_STRING && col.kind != WR_DECIMAL) {
    if (threadIdx.x == 0) blen[j] = 0;
    return;
  }
  const uint64_t v0 = vscan[j] - vscan[c * G], n = cnt[j];
  uint64_t b = 0;
  if (col.kind == WR_DECIMAL) {  // Decimal128: the varints' bytes
    const uint64_t* q = (const uint64_t*)col.vals;
    for (uint64_t i = threadIdx.x; i < n; i += 256) b += wr_dec_varint_len(wr_dec_zigzag(q[2 * (v0 + i)], q[2 * (v0 + i) + 1]));
  } else {
    for (uint64_t i = threadIdx.x; i < n; i += 256) b += ix_len(col.vals, col.elem, v0 + i);
  }
  b = ix_block_sum(b, lds);
  if (threadIdx.x == 0) blen[j] = b;
}

// ---- double-double sums (no contraction: the error terms must be exact) ------------------------------------------------------
__device__ __forceinline__ void ix_two_sum(double a, double b, double& s, double& e) {
#pragma clang fp contract(off)
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}
__device__ __forceinline__ void ix_dd_add(double& hi, double& lo, double x) {
  double s, e;
  ix_two_sum(hi, x, s, e);
  hi = s;
  lo += e;
}
__device__ __forceinline__ void ix_dd_merge(double& hi, double& lo, double h2, double l2) {
#pragma clang fp contract(off)
  double s, e;
  ix_two_sum(hi, h2, s, e);
  e += lo + l2;
  hi = s + e;
  lo = e - (hi - s);
}
// a double-double's merge where either may be infinite or NaN (then the sum is what any order gives)
__device__ __forceinline__ void ix_dd_merge_inf(double& hi, double& lo, double h2, double l2) {
  if (__builtin_isfinite(hi) && __builtin_isfinite(h2)) ix_dd_merge(hi, lo, h2, l2);
  else hi = hi + h2, lo = 0;
}
#define IX_BIG 0x1p960         // float values at or above this magnitude are summed apart, scaled by IX_BIG_SCALE
#define IX_BIG_SCALE 0x1p-64

// strings: the first 8 bytes, big-endian, zero-padded
__device__ __forceinline__ uint64_t ix_key(const uint8_t* p, uint32_t len) {
  uint64_t k = 0;
  for (uint32_t i = 0; i < 8; i++) k = (k << 8) | (i < len ? p[i] : 0u);
  return k;
}
// < 0: a before b by bytes (a prefix first); the keys are compared first, the bytes only past them
__device__ int ix_strcmp(const uint8_t* data, uint64_t a, uint32_t la, uint64_t ka, uint64_t b, uint32_t lb, uint64_t kb) {
  if (ka != kb) return ka < kb ? -1 : 1;
  const uint32_t n = min(la, lb);
  for (uint32_t i = 8; i < n; i++) {
    const uint8_t x = data[a + i], y = data[b + i];
    if (x != y) return x < y ? -1 : 1;
  }
  return la < lb ? -1 : (la > lb ? 1 : 0);
}

#define IX_NONE 0xffffffffu

extern "C" __global__ void __launch_bounds__(256) ix_stats_kernel(const IxCol* cols, uint64_t rows, uint64_t S, uint64_t G, const uint64_t* cnt,
                                                                  const uint64_t* vscan, const uint64_t* bscan, IxRec* recs, uint64_t* side_len) {
  __shared__ uint64_t l0[256], l1[256], l2[256];
  __shared__ uint64_t m0[256], m1[256], m2[256];
  __shared__ uint32_t n0[256], n1[256];
  __shared__ double b0[256], b1[256];
  const uint32_t t = threadIdx.x;
  const uint64_t j = blockIdx.x, c = j / G, g = j % G;
  const IxCol col = cols[c];
  const uint64_t r0 = g * S, r1 = min(r0 + S, rows);
  const uint64_t v0 = vscan[j] - vscan[c * G], n = cnt[j];
  IxRec R = {};
  R.count = n;
  R.has_null = n < r1 - r0;
  if (col.kind == WR_INT || col.kind == WR_BYTE) {  // integers: min, max, exact sum
    int64_t mn = INT64_MAX, mx = INT64_MIN;
    __int128 sum = 0;
    for (uint64_t i = t; i < n; i += 256) {
      const uint64_t k = v0 + i;
      int64_t x;
      switch (col.elem) {
        case 1: x = ((const int8_t*)col.vals)[k]; break;
        case 2: x = ((const int16_t*)col.vals)[k]; break;
        case 4: x = ((const int32_t*)col.vals)[k]; break;
        default: x = ((const int64_t*)col.vals)[k]; break;
      }
      mn = min(mn, x);
      mx = max(mx, x);
      sum += x;
    }
    l0[t] = (uint64_t)mn;
    l1[t] = (uint64_t)mx;
    m0[t] = (uint64_t)sum;
    m1[t] = (uint64_t)(sum >> 64);
    __syncthreads();
    for (uint32_t d = 128; d > 0; d >>= 1) {
      if (t < d) {
        l0[t] = (uint64_t)min((int64_t)l0[t], (int64_t)l0[t + d]);
        l1[t] = (uint64_t)max((int64_t)l1[t], (int64_t)l1[t + d]);
        const unsigned __int128 a = ((unsigned __int128)m1[t] << 64) | m0[t], b = ((unsigned __int128)m1[t + d] << 64) | m0[t + d];
        const unsigned __int128 s = a + b;
        m0[t] = (uint64_t)s;
        m1[t] = (uint64_t)(s >> 64);
      }
      __syncthreads();
    }
    R.imin = (int64_t)l0[0];
    R.imax = (int64_t)l1[0];
    R.sum_lo = m0[0];
    R.sum_hi = (int64_t)m1[0];
  } else if (col.kind == WR_FLOAT) {  // floats as f64: min / max (the first of equal values, as a sequential writer keeps it), NaN, sum
    // The sum is two double-doubles: values below 2^960 in magnitude, and the others scaled by 2^-64 (exact for them).  Neither
    // can overflow for fewer than 2^63 values, so the sum does not depend on the order (the host adds them: wr_stat_msg); an
    // infinite input makes the second one infinite.
    double mn = 0, mx = 0, hi = 0, lo = 0, bhi = 0, blo = 0;
    uint64_t imn = ~0ull, imx = ~0ull;
    uint32_t nan = 0;
    for (uint64_t i = t; i < n; i += 256) {
      const uint64_t k = v0 + i;
      const double x = col.elem == 4 ? (double)((const float*)col.vals)[k] : ((const double*)col.vals)[k];
      if (x != x) {
        nan = 1;
        continue;
      }
      if (imn == ~0ull || x < mn) mn = x, imn = i;
      if (imx == ~0ull || x > mx) mx = x, imx = i;
      if (__builtin_fabs(x) < IX_BIG) ix_dd_add(hi, lo, x);
      else if (__builtin_isfinite(bhi)) ix_dd_add(bhi, blo, x * IX_BIG_SCALE);
      else bhi += x;
    }
    double* d0 = (double*)l0;
    double* d1 = (double*)l1;
    double* dh = (double*)m0;
    double* dl = (double*)m1;
    d0[t] = mn;
    d1[t] = mx;
    l2[t] = imn;
    m2[t] = imx;
    dh[t] = hi;
    dl[t] = lo;
    n0[t] = nan;
    b0[t] = bhi;
    b1[t] = blo;
    __syncthreads();
    for (uint32_t d = 128; d > 0; d >>= 1) {
      if (t < d) {
        const uint64_t ia = l2[t], ib = l2[t + d];
        if (ib != ~0ull && (ia == ~0ull || d0[t + d] < d0[t] || (d0[t + d] == d0[t] && ib < ia))) d0[t] = d0[t + d], l2[t] = ib;
        const uint64_t xa = m2[t], xb = m2[t + d];
        if (xb != ~0ull && (xa == ~0ull || d1[t + d] > d1[t] || (d1[t + d] == d1[t] && xb < xa))) d1[t] = d1[t + d], m2[t] = xb;
        double h = dh[t], l = dl[t], bh = b0[t], bl = b1[t];
        ix_dd_merge(h, l, dh[t + d], dl[t + d]);
        ix_dd_merge_inf(bh, bl, b0[t + d], b1[t + d]);
        dh[t] = h;
        dl[t] = l;
        b0[t] = bh;
        b1[t] = bl;
        n0[t] |= n0[t + d];
      }
      __syncthreads();
    }
    R.dmin = d0[0];
    R.dmax = d1[0];
    R.dsum = dh[0];
    R.dsum_lo = dl[0];
    R.dbig = b0[0];
    R.dbig_lo = b1[0];
    R.has_nan = n0[0];
  } else if (col.kind == WR_BOOL) {  // Boolean: trues
    uint64_t tr = 0;
    for (uint64_t i = t; i < n; i += 256) tr += ((const uint8_t*)col.vals)[v0 + i];
    R.trues = ix_block_sum(tr, l0);
  } else if (col.kind == WR_TIMESTAMP) {  // Timestamp: minimum and maximum by (second, nanosecond)
    int64_t s0 = INT64_MAX, s1 = INT64_MIN;
    uint32_t q0 = 0xffffffffu, q1 = 0;
    for (uint64_t i = t; i < n; i += 256) {
      int64_t S;
      uint32_t N;
      wr_timestamp_of(((const int64_t*)col.vals)[v0 + i], ((const uint64_t*)col.data)[v0 + i], S, N);
      if (S < s0 || (S == s0 && N < q0)) s0 = S, q0 = N;
      if (S > s1 || (S == s1 && N > q1)) s1 = S, q1 = N;
    }
    l0[t] = (uint64_t)s0, l1[t] = (uint64_t)s1, n0[t] = q0, n1[t] = q1;
    __syncthreads();
    for (uint32_t d = 128; d > 0; d >>= 1) {
      if (t < d) {
        const int64_t a0 = (int64_t)l0[t + d], a1 = (int64_t)l1[t + d];
        if (a0 < (int64_t)l0[t] || (a0 == (int64_t)l0[t] && n0[t + d] < n0[t])) l0[t] = l0[t + d], n0[t] = n0[t + d];
        if (a1 > (int64_t)l1[t] || (a1 == (int64_t)l1[t] && n1[t + d] > n1[t])) l1[t] = l1[t + d], n1[t] = n1[t + d];
      }
      __syncthreads();
    }
    R.imin = (int64_t)l0[0];
    R.imax = (int64_t)l1[0];
    R.sum_lo = n0[0];
    R.sum_hi = n1[0];
  } else if (col.kind == WR_DECIMAL) {  // Decimal128: minimum, maximum, and the exact sum in 192 bits (fewer than 2^32 values below 2^127)
    const uint64_t* q = (const uint64_t*)col.vals;
    __int128 mn = 0, mx = 0;
    uint64_t s0 = 0, s1 = 0, s2 = 0;
    bool any = false;
    for (uint64_t i = t; i < n; i += 256) {
      const uint64_t lo = q[2 * (v0 + i)], hi = q[2 * (v0 + i) + 1];
      const __int128 x = (__int128)(((unsigned __int128)hi << 64) | lo);
      if (!any || x < mn) mn = x;
      if (!any || x > mx) mx = x;
      any = true;
      const unsigned __int128 lo2 = (unsigned __int128)s0 + lo;
      const unsigned __int128 mid = (unsigned __int128)s1 + hi + (uint64_t)(lo2 >> 64);
      s0 = (uint64_t)lo2;
      s1 = (uint64_t)mid;
      s2 += (uint64_t)((int64_t)hi >> 63) + (uint64_t)(mid >> 64);
    }
    uint64_t* sx = (uint64_t*)b0;
    uint64_t* ok = (uint64_t*)b1;
    l0[t] = (uint64_t)mn, l1[t] = (uint64_t)((unsigned __int128)mn >> 64);
    l2[t] = (uint64_t)mx, m0[t] = (uint64_t)((unsigned __int128)mx >> 64);
    m1[t] = s0, m2[t] = s1, sx[t] = s2, ok[t] = any;
    __syncthreads();
    for (uint32_t d = 128; d > 0; d >>= 1) {
      if (t < d) {
        if (ok[t + d]) {
          const __int128 a = (__int128)(((unsigned __int128)l1[t] << 64) | l0[t]), b = (__int128)(((unsigned __int128)l1[t + d] << 64) | l0[t + d]);
          const __int128 e = (__int128)(((unsigned __int128)m0[t] << 64) | l2[t]), f = (__int128)(((unsigned __int128)m0[t + d] << 64) | l2[t + d]);
          if (!ok[t] || b < a) l0[t] = l0[t + d], l1[t] = l1[t + d];
          if (!ok[t] || f > e) l2[t] = l2[t + d], m0[t] = m0[t + d];
          ok[t] = 1;
        }
        const unsigned __int128 lo2 = (unsigned __int128)m1[t] + m1[t + d];
        const unsigned __int128 mid = (unsigned __int128)m2[t] + m2[t + d] + (uint64_t)(lo2 >> 64);
        m1[t] = (uint64_t)lo2;
        m2[t] = (uint64_t)mid;
        sx[t] += sx[t + d] + (uint64_t)(mid >> 64);
      }
      __syncthreads();
    }
    R.imin = (int64_t)l0[0];
    R.imax = (int64_t)l1[0];
    R.smin_at = l2[0];
    R.smax_at = m0[0];
    R.sum_lo = m1[0];
    R.sum_hi = (int64_t)m2[0];
    R.trues = sx[0];
  } else {  // strings / binaries: bytes; Utf8: min and max by bytes
    const uint64_t b0 = bscan[j] - bscan[c * G];
    R.bytes = bscan[j + 1] - bscan[j];
    if (col.minmax && n) {
      uint64_t amn = 0, amx = 0, kmn = 0, kmx = 0;
      uint32_t lmn = IX_NONE, lmx = IX_NONE;
      uint64_t base = b0;  // the bytes before this chunk of 256 values
      for (uint64_t i0 = 0; i0 < n; i0 += 256) {
        const uint64_t i = i0 + t;
        const uint32_t len = i < n ? (uint32_t)ix_len(col.vals, col.elem, v0 + i) : 0;
        // exclusive scan of the chunk's lengths
        l2[t] = len;
        __syncthreads();
        for (uint32_t d = 1; d < 256; d *= 2) {
          const uint64_t a = t >= d ? l2[t - d] : 0;
          __syncthreads();
          l2[t] += a;
          __syncthreads();
        }
        const uint64_t at = base + l2[t] - len;
        const uint64_t chunk = l2[255];
        __syncthreads();
        base += chunk;
        if (i < n) {
          const uint64_t k = ix_key(col.data + at, len);
          if (lmn == IX_NONE || ix_strcmp(col.data, at, len, k, amn, lmn, kmn) < 0) amn = at, lmn = len, kmn = k;
          if (lmx == IX_NONE || ix_strcmp(col.data, at, len, k, amx, lmx, kmx) > 0) amx = at, lmx = len, kmx = k;
        }
      }
      l0[t] = amn, l1[t] = kmn, n0[t] = lmn;
      m0[t] = amx, m1[t] = kmx, n1[t] = lmx;
      __syncthreads();
      for (uint32_t d = 128; d > 0; d >>= 1) {
        if (t < d) {
          if (n0[t + d] != IX_NONE && (n0[t] == IX_NONE || ix_strcmp(col.data, l0[t + d], n0[t + d], l1[t + d], l0[t], n0[t], l1[t]) < 0))
            l0[t] = l0[t + d], l1[t] = l1[t + d], n0[t] = n0[t + d];
          if (n1[t + d] != IX_NONE && (n1[t] == IX_NONE || ix_strcmp(col.data, m0[t + d], n1[t + d], m1[t + d], m0[t], n1[t], m1[t]) > 0))
            m0[t] = m0[t + d], m1[t] = m1[t + d], n1[t] = n1[t + d];
        }
        __syncthreads();
      }
      R.smin_at = l0[0];
      R.smin_len = n0[0];
      R.smax_at = m0[0];
      R.smax_len = n1[0];
    }
  }
  if (t == 0) {
    recs[j] = R;
    side_len[j] = col.kind == WR_STRING && col.minmax && n ? min(R.smin_len, IX_STR_KEEP) + min(R.smax_len, IX_STR_KEEP) : 0;
  }
}

extern "C" __global__ void __launch_bounds__(256) ix_side_kernel(const IxCol* cols, uint64_t G, const uint64_t* side_off, IxRec* recs, uint8_t* side) {
  const uint64_t j = blockIdx.x, c = j / G;
  const IxCol col = cols[c];
  if (col.kind != WR_STRING || !col.minmax) return;
  const IxRec& R = recs[j];
  if (!R.count) return;
  const uint64_t o = side_off[j];
  const uint32_t a = min(R.smin_len, IX_STR_KEEP), b = min(R.smax_len, IX_STR_KEEP);
  for (uint32_t i = threadIdx.x; i < a; i += 256) side[o + i] = col.data[R.smin_at + i];
  for (uint32_t i = threadIdx.x; i < b; i += 256) side[o + a + i] = col.data[R.smax_at + i];
  if (threadIdx.x == 0) recs[j].side = o;
}

// One stream of a column: pos[g * 4 ..] = {byte offset, 0, values of the run consumed, bits of the byte consumed} where group g
// starts.  mode: 0 PRESENT (bits over byte runs, from row g * S), 1 Integer RLE v2, 2 byte RLE, 3 Boolean DATA (bits over byte
// runs), 4 floats (elem bytes a value), 5 string bytes.  vscan / bscan: the column's jobs (group g at [g]).  n: values of the
// stream (PRESENT: rows).  A group that starts past the last value points at the stream's end with nothing consumed.
extern "C" __global__ void __launch_bounds__(256) ix_pos_kernel(int mode, uint64_t G, uint64_t S, const uint64_t* vscan, const uint64_t* bscan, uint64_t n, int elem,
                                                                const uint32_t* runs, const uint64_t* offsets, const uint64_t* d_n_runs,
                                                                const uint64_t* d_total, uint64_t* pos) {
  const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  uint64_t* p = pos + g * 4;
  const uint64_t v = mode == 0 ? g * S : vscan[g] - vscan[0];
  uint64_t u = 0, vals = 0, bits = 0;
  if (mode == 4) {
    u = v * (uint64_t)elem;
  } else if (mode == 5) {
    u = bscan[g] - bscan[0];
  } else {
    const bool bit = mode == 0 || mode == 3;
    const uint64_t x = bit ? v / 8 : v, xn = bit ? (n + 7) / 8 : n;
    if (x >= xn) {
      u = xn ? *d_total : 0;
    } else {
      const uint32_t n_runs = (uint32_t)*d_n_runs;
      uint32_t lo = 0, hi = n_runs;  // the last run starting at or before x
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (runs[mid] <= x) lo = mid;
        else hi = mid;
      }
      u = offsets[lo];
      vals = x - runs[lo];
      bits = bit ? v % 8 : 0;
    }
  }
  p[0] = u;
  p[1] = 0;
  p[2] = vals;
  p[3] = bits;
}

// compressed file: every stream s's positions [s * G .. (s + 1) * G) from uncompressed offsets to the compressed stream's
// (chunk header, bytes into it), with the chunk table the compressor left (lzc_plan_kernel, the scan of lzc_chunk_size_kernel)
extern "C" __global__ void __launch_bounds__(256) ix_map_kernel(uint64_t n_slots, uint64_t G, uint64_t B, const LzcPlan* plan, const uint64_t* chunk_off,
                                                                uint64_t* pos) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_slots) return;
  const uint64_t s = i / G;
  uint64_t* p = pos + i * 4;
  const uint64_t u = p[0], first = plan[s].chunk0, nch = plan[s + 1].chunk0 - first;
  const uint64_t k = min(u / B, nch);
  p[0] = chunk_off[first + k] - chunk_off[first];
  p[1] = u - k * B;
}
