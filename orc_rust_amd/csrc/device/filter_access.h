// filter_access.h -- row access over a decoded stripe, for every kernel that reads rows where the decode left them: the row
// filter's kernels (filter_kernels.hip) and the aggregation's (agg_kernels.hip).
//
// The input rows are the result's rows as its batches hand them out: all rows of the stripe (n_segs = 0), or the row ranges
// of a row selection (SelBatch segments).  The stripe-wide buffers of the decode are read the way select_build_kernel does:
// uniform batches of `B` rows, `W` validity words per batch, string offsets that restart per batch plus the batch's char base.
// All of that is written down once, here (filter_row .. filter_value_str): a kernel addresses a row through these helpers only.
// The aggregation's kernels take what filter_row needs, with the columns and the keep mask, as one argument: KeptRows.
#pragma once
#include <stdint.h>

struct FilterCol {
  const unsigned long long* validity;   // per uniform batch W words (null: no PRESENT stream, every row is valid)
  const uint8_t* values;                // fixed width: row * width; Boolean: bit words laid out like validity
  const int32_t* offsets;               // strings: per uniform batch B + 1 offsets restarting at 0
  const unsigned long long* char_base;  // strings: byte position of every uniform batch's first value byte
  const uint8_t* chars;                 // strings: the stripe's value bytes
  uint32_t width;                       // fixed width in bytes
  uint32_t kind;                        // FKIND_*
};

// input row j -> row of the stripe (n_segs = 0: the identity)
__device__ __forceinline__ uint64_t filter_src_row(const SelBatch* segs, const unsigned long long* seg_first, uint32_t n_segs, uint64_t j) {
  if (!n_segs) return j;
  uint32_t lo = 0, hi = n_segs - 1;  // the last segment whose first input row is <= j
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (seg_first[mid] <= j) lo = mid;
    else hi = mid - 1;
  }
  return segs[lo].start + (j - seg_first[lo]);
}

// ---- row access: how every kernel finds a row and loads what a column holds for it ----
// A row of the stripe as the decode laid it out: uniform batch u, row l of it
struct FilterRow {
  bool live;  // false: an input row past n_in (row = u = l = 0 then: loads stay in bounds, their results are masked out)
  uint64_t row, u;
  uint32_t l;
};
__device__ __forceinline__ FilterRow filter_row_of(uint64_t row, uint32_t B, bool live = true) {
  return {live, row, row / B, (uint32_t)(row % B)};
}
__device__ __forceinline__ FilterRow filter_row(const SelBatch* segs, const unsigned long long* seg_first, uint32_t n_segs, uint64_t n_in, uint32_t B,
                                                uint64_t j) {
  return filter_row_of(j < n_in ? filter_src_row(segs, seg_first, n_segs, j) : 0, B, j < n_in);
}
// The 64-bit words of a mask over the input rows (`keep`, a plane), dealt to the wavefronts of a grid of 256-thread blocks:
//   for (uint64_t w = ws.first; w < ws.n; w += ws.stride) { input row j = w * 64 + lane ... }
struct FilterWords {
  uint64_t first, stride, n;
};
__device__ __forceinline__ FilterWords filter_words(uint64_t n_in) {
  return {(uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), (uint64_t)gridDim.x * 4, (n_in + 63) / 64};
}

// The rows a kernel walks, as ONE kernel argument passed by value (the aggregation's kernels; the host builds it once per call):
// the columns, the input rows' segments, and the keep mask filter_eval_kernel left -- one word per 64 input rows; null: no filter,
// every input row is kept.  Behind it the planes of the aggregates' conditions (agg_cond_eval_kernel): n_cond of them, each laid
// out like `keep`, plane k at cond + k * ceil(n_in / 64) -- bit = the row is kept and condition k is TRUE for it; none: null, 0
struct KeptRows {
  const FilterCol* cols;
  const SelBatch* segs;
  const unsigned long long* seg_first;
  uint32_t n_segs;
  uint64_t n_in;
  uint32_t B, W;
  const unsigned long long* keep;
  const unsigned long long* cond;
  uint32_t n_cond;
};
__device__ __forceinline__ FilterRow filter_row(const KeptRows& rows, uint64_t j) {
  return filter_row(rows.segs, rows.seg_first, rows.n_segs, rows.n_in, rows.B, j);
}

// bit l of batch u in bit words laid out per uniform batch (validity, Boolean values)
__device__ __forceinline__ bool filter_bit(const unsigned long long* w, uint64_t u, uint32_t l, uint32_t W) { return (w[u * W + (l >> 6)] >> (l & 63)) & 1; }
__device__ __forceinline__ bool filter_valid(const FilterCol& c, uint64_t u, uint32_t l, uint32_t W) {
  return !c.validity || filter_bit(c.validity, u, l, W);
}
__device__ __forceinline__ bool filter_load_bit(const FilterCol& c, uint64_t u, uint32_t l, uint32_t W) {
  return filter_bit(reinterpret_cast<const unsigned long long*>(c.values), u, l, W);
}
__device__ __forceinline__ long long filter_load_i64(const FilterCol& c, uint64_t row) {
  if (c.width == 1) return reinterpret_cast<const int8_t*>(c.values)[row];
  if (c.width == 2) return reinterpret_cast<const int16_t*>(c.values)[row];
  if (c.width == 4) return reinterpret_cast<const int32_t*>(c.values)[row];
  return reinterpret_cast<const long long*>(c.values)[row];
}
__device__ __forceinline__ double filter_load_f64(const FilterCol& c, uint64_t row) {
  return c.width == 4 ? (double)reinterpret_cast<const float*>(c.values)[row] : reinterpret_cast<const double*>(c.values)[row];
}
// one 16-byte load (row * 16 off a 256-byte aligned arena), little-endian halves
__device__ __forceinline__ void filter_load_dec128(const FilterCol& c, uint64_t row, unsigned long long* lo, unsigned long long* hi) {
  const uint4 q = reinterpret_cast<const uint4*>(c.values)[row];
  *lo = ((unsigned long long)q.y << 32) | q.x;
  *hi = ((unsigned long long)q.w << 32) | q.z;
}
// A string value by its offsets pair alone -- o[0], o[1] of filter_str_offsets --: where it starts among its batch's bytes, and
// its length
struct FilterSpan {
  uint32_t start, len;
};
__device__ __forceinline__ const int32_t* filter_str_offsets(const FilterCol& c, uint64_t u, uint32_t l, uint32_t B) {
  return c.offsets + u * (B + 1) + l;
}
__device__ __forceinline__ FilterSpan filter_str_span(const FilterCol& c, uint64_t u, uint32_t l, uint32_t B) {
  const int32_t* o = filter_str_offsets(c, u, l, B);
  const uint32_t a = (uint32_t)o[0];
  return {a, (uint32_t)o[1] - a};
}
__device__ __forceinline__ uint32_t filter_str_len(const FilterCol& c, uint64_t u, uint32_t l, uint32_t B) { return filter_str_span(c, u, l, B).len; }
// A string value: its bytes p[0, len).  The chars buffer promises nothing behind its last value: whoever loads p[x] keeps x < len.
// From a span already loaded (whoever decides by the length alone loads no char base for the values it passes over), or from the row.
struct FilterStr {
  const uint8_t* p;
  uint32_t len;
};
__device__ __forceinline__ FilterStr filter_value_str(const FilterCol& c, uint64_t u, FilterSpan s) { return {c.chars + c.char_base[u] + s.start, s.len}; }
__device__ __forceinline__ FilterStr filter_value_str(const FilterCol& c, uint64_t u, uint32_t l, uint32_t B) {
  return filter_value_str(c, u, filter_str_span(c, u, l, B));
}
