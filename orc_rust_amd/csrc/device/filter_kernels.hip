// filter_kernels.hip -- a ROW FILTER over a decoded stripe: per-row predicate evaluation and a compacting gather.
//
// The reference has no row-level evaluation (its predicates prune row groups only, row_group_filter.rs); the semantics are
// those of include/orcgpu.h (orcgpu_result_filter): SQL three-valued logic, a row is kept when the root is TRUE.
//
//   filter_eval_kernel    one lane per input row, one 64-bit word of the keep mask per wavefront trip.  The predicate is a
//                         post-order program (FilterInsn); a leaf yields two ballot words for the trip's 64 rows -- the rows
//                         where it is TRUE and the rows where it is FALSE (neither: UNKNOWN) --, inner nodes combine words on
//                         a per-wavefront stack with wave-uniform code.  Writes keep = T_root & live and its popcount.
//                         A Decimal leaf compares the row's 16 bytes with a literal the host has brought to the column's scale,
//                         a Timestamp leaf is the integer leaf on a literal in the column's unit: no row is ever rescaled.
//   (enc_scan)            exclusive scan of the popcounts: the output row of every word's first kept row.
//   filter_place_kernel   every kept row writes its stripe row at its output row: src_rows[], the gather's index list.
//   filter_count_kernel   per (output batch, column): null count and string bytes -- what the host needs to lay the output out
//                         compactly; it is fetched with the row count in the filter's ONE host wait.
//   filter_gather_kernel  per (output batch, column): fixed-width values (16-byte stores where the batch's first value is
//                         16-byte aligned), Boolean bits and validity rebuilt by ballot, string lengths -> offsets restarting
//                         at 0 (a block scan) -> bytes (a lane per short value, a wavefront per long one).
//
// The input rows are the result's rows as its batches hand them out: all rows of the stripe (n_segs = 0), or the row ranges
// of a row selection (SelBatch segments).  Leaves and the gather read the stripe-wide buffers of the decode the way
// select_build_kernel does: uniform batches of `B` rows, `W` validity words per batch, string offsets that restart per
// batch plus the batch's char base.  Output rows [k * B, (k + 1) * B) form output batch k.
#pragma once
#include <stdint.h>

#include "filter_program.h"

struct FilterCol {
  const unsigned long long* validity;   // per uniform batch W words (null: no PRESENT stream, every row is valid)
  const uint8_t* values;                // fixed width: row * width; Boolean: bit words laid out like validity
  const int32_t* offsets;               // strings: per uniform batch B + 1 offsets restarting at 0
  const unsigned long long* char_base;  // strings: byte position of every uniform batch's first value byte
  const uint8_t* chars;                 // strings: the stripe's value bytes
  uint32_t width;                       // fixed width in bytes
  uint32_t kind;                        // FKIND_*
};

struct FilterGatherJob {
  FilterCol src;
  unsigned long long* out_validity;           // per output batch W words (null: the kept rows hold no null)
  uint8_t* out_values;                        // fixed width: output row * width; Boolean: W words per output batch
  int32_t* out_offsets;                       // strings: per output batch B + 1
  uint8_t* out_chars;                         // strings: the kept rows' bytes, batch after batch
  const unsigned long long* out_char_base;    // strings: per output batch, where its bytes start in out_chars
};

constexpr uint32_t kFilterShortString = 32;    // values up to this many bytes are copied by one lane, longer ones by a wavefront

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

__device__ __forceinline__ bool filter_valid(const FilterCol& c, uint64_t u, uint32_t l, uint32_t W) {
  return !c.validity || ((c.validity[u * W + (l >> 6)] >> (l & 63)) & 1);
}
__device__ __forceinline__ uint32_t filter_str_len(const FilterCol& c, uint64_t u, uint32_t l, uint32_t B) {
  const int32_t* o = c.offsets + u * (B + 1) + l;
  return (uint32_t)o[1] - (uint32_t)o[0];
}

extern "C" __global__ void __launch_bounds__(256)
filter_eval_kernel(const FilterInsn* prog, uint32_t n_insn, const uint8_t* lits, const FilterCol* cols, const SelBatch* segs,
                   const unsigned long long* seg_first, uint32_t n_segs, uint64_t n_in, uint32_t B, uint32_t W, unsigned long long* keep,
                   uint32_t* cnt) {
  __shared__ unsigned long long stk_t[4][kFilterStack], stk_f[4][kFilterStack];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t n_words = (n_in + 63) / 64;
  for (uint64_t w = (uint64_t)blockIdx.x * 4 + wave; w < n_words; w += (uint64_t)gridDim.x * 4) {
    const uint64_t j = w * 64 + lane;
    const bool live = j < n_in;
    const uint64_t row = live ? filter_src_row(segs, seg_first, n_segs, j) : 0;
    const uint64_t u = row / B;
    const uint32_t l = (uint32_t)(row % B);
    const unsigned long long live_m = __ballot(live);
    uint32_t sp = 0;
    for (uint32_t k = 0; k < n_insn; k++) {
      const FilterInsn in = prog[k];
      unsigned long long T = 0, F = 0;
      if (in.op <= FOP_IS_NOT_NULL) {
        const FilterCol c = cols[in.col];
        const bool valid = live && filter_valid(c, u, l, W);
        bool t = false, f = false;
        if (in.op == FOP_IS_NULL) {
          t = live && !valid;
          f = valid;
        } else if (in.op == FOP_IS_NOT_NULL) {
          t = valid;
          f = live && !valid;
        } else if (valid) {
          bool lt = false, eq = false, gt = false;
          if (in.op == FOP_CMP_INT) {
            long long v;
            if (c.width == 1) v = reinterpret_cast<const int8_t*>(c.values)[row];
            else if (c.width == 2) v = reinterpret_cast<const int16_t*>(c.values)[row];
            else if (c.width == 4) v = reinterpret_cast<const int32_t*>(c.values)[row];
            else v = reinterpret_cast<const long long*>(c.values)[row];
            lt = v < in.i;
            eq = v == in.i;
            gt = v > in.i;
          } else if (in.op == FOP_CMP_FLOAT) {
            const double v = c.width == 4 ? (double)reinterpret_cast<const float*>(c.values)[row] : reinterpret_cast<const double*>(c.values)[row];
            lt = v < in.f;
            eq = v == in.f;
            gt = v > in.f;
          } else if (in.op == FOP_CMP_BOOL) {
            const long long v = (long long)((reinterpret_cast<const unsigned long long*>(c.values)[u * W + (l >> 6)] >> (l & 63)) & 1);
            lt = v < in.i;
            eq = v == in.i;
            gt = v > in.i;
          } else if (in.op == FOP_CMP_DEC128) {
            // one 16-byte load (row * 16 off a 256-byte aligned arena); the high words as signed, the low words as unsigned
            const uint4 q = reinterpret_cast<const uint4*>(c.values)[row];
            const long long vh = (long long)(((unsigned long long)q.w << 32) | q.z);
            const unsigned long long vl = ((unsigned long long)q.y << 32) | q.x;
            eq = vh == in.i && vl == in.lo;
            lt = vh < in.i || (vh == in.i && vl < in.lo);
            gt = !lt && !eq;
          } else {  // FOP_CMP_STRING
            const int32_t* o = c.offsets + u * (B + 1) + l;
            const uint32_t a = (uint32_t)o[0], len = (uint32_t)o[1] - a;
            const uint8_t* p = c.chars + c.char_base[u] + a;
            const uint8_t* q = lits + in.lit_off;
            const uint32_t m = len < in.lit_len ? len : in.lit_len;
            uint32_t x = 0;
            while (x < m && p[x] == q[x]) x++;
            if (x < m) {
              lt = p[x] < q[x];
              gt = !lt;
            } else {
              lt = len < in.lit_len;
              eq = len == in.lit_len;
              gt = len > in.lit_len;
            }
          }
          switch (in.cmp) {
            case 0: t = eq; break;         // EQ
            case 1: t = !eq; break;        // NE (true with a NaN on either side)
            case 2: t = lt; break;         // LT
            case 3: t = lt || eq; break;   // LE
            case 4: t = gt; break;         // GT
            default: t = gt || eq; break;  // GE
          }
          f = !t;
        }
        T = __ballot(t);
        F = __ballot(f);
      } else if (in.op == FOP_TRUE) {
        T = live_m;
      } else if (in.op == FOP_FALSE) {
        F = live_m;
      } else if (in.op == FOP_NOT) {
        sp--;
        T = stk_f[wave][sp];
        F = stk_t[wave][sp];
      } else if (in.op == FOP_AND || in.op == FOP_OR) {
        sp -= 2;
        const unsigned long long t1 = stk_t[wave][sp], f1 = stk_f[wave][sp], t2 = stk_t[wave][sp + 1], f2 = stk_f[wave][sp + 1];
        if (in.op == FOP_AND) {
          T = t1 & t2;
          F = f1 | f2;
        } else {
          T = t1 | t2;
          F = f1 & f2;
        }
      }  // (FOP_UNKNOWN: neither)
      // (every lane holds the same words and writes them to the same slot: the wavefront's stack needs no barrier)
      stk_t[wave][sp] = T;
      stk_f[wave][sp] = F;
      sp++;
    }
    const unsigned long long root = (sp ? stk_t[wave][0] : 0ull) & live_m;
    if (lane == 0) {
      keep[w] = root;
      cnt[w] = (uint32_t)__builtin_popcountll(root);
    }
  }
}

// every kept input row -> src_rows[its output row] = its row of the stripe
extern "C" __global__ void __launch_bounds__(256)
filter_place_kernel(const unsigned long long* keep, const unsigned long long* woff, const SelBatch* segs, const unsigned long long* seg_first,
                    uint32_t n_segs, uint64_t n_in, uint32_t* src_rows) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_in) return;
  const unsigned long long m = keep[j >> 6];
  const uint32_t lane = (uint32_t)(j & 63);
  if (!((m >> lane) & 1)) return;
  const uint64_t o = woff[j >> 6] + (uint64_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
  src_rows[o] = (uint32_t)filter_src_row(segs, seg_first, n_segs, j);
}

// blockIdx.x = output batch (of at most nb_max; those past the kept rows leave at once), blockIdx.y = column.
// nulls / char_total: [column][nb_max], zeroed by the host
extern "C" __global__ void __launch_bounds__(256)
filter_count_kernel(const FilterCol* cols, const uint32_t* src_rows, const unsigned long long* total, uint32_t B, uint32_t W, uint32_t nb_max,
                    unsigned long long* nulls, unsigned long long* char_total) {
  const FilterCol c = cols[blockIdx.y];
  const uint64_t kept = *total, first = (uint64_t)blockIdx.x * B;
  if (first >= kept || (!c.validity && c.kind != FKIND_STRING)) return;
  const uint32_t len = (uint32_t)(kept - first < B ? kept - first : B);
  unsigned long long n_null = 0, n_bytes = 0;
  for (uint32_t i = threadIdx.x; i < len; i += 256) {
    const uint64_t row = src_rows[first + i];
    const uint64_t u = row / B;
    const uint32_t l = (uint32_t)(row % B);
    if (!filter_valid(c, u, l, W)) n_null++;
    if (c.kind == FKIND_STRING) n_bytes += filter_str_len(c, u, l, B);
  }
  for (int o = 32; o; o >>= 1) {
    n_null += (unsigned long long)__shfl_xor((long long)n_null, o);
    n_bytes += (unsigned long long)__shfl_xor((long long)n_bytes, o);
  }
  if ((threadIdx.x & 63) == 0) {
    const uint64_t at = (uint64_t)blockIdx.y * nb_max + blockIdx.x;
    if (n_null) atomicAdd(&nulls[at], n_null);
    if (n_bytes) atomicAdd(&char_total[at], n_bytes);
  }
}

// `len` values of type T from rows[] of src to contiguous out: 16-byte stores (16 / sizeof(T) values a lane) when out is 16-byte
// aligned, the tail and unaligned batches value by value
template <typename T>
__device__ __forceinline__ void filter_gather_fixed(const uint8_t* src_, uint8_t* out_, const uint32_t* rows, uint32_t len) {
  const T* src = reinterpret_cast<const T*>(src_);
  T* out = reinterpret_cast<T*>(out_);
  constexpr uint32_t R = 16 / sizeof(T);
  uint32_t done = 0;
  if ((reinterpret_cast<uintptr_t>(out_) & 15) == 0) {
    const uint32_t groups = len / R;
    for (uint32_t g = threadIdx.x; g < groups; g += 256) {
      union {
        T v[R];
        uint4 q;
      } x;
#pragma unroll
      for (uint32_t r = 0; r < R; r++) x.v[r] = src[rows[g * R + r]];
      reinterpret_cast<uint4*>(out_)[g] = x.q;
    }
    done = groups * R;
  }
  for (uint32_t i = done + threadIdx.x; i < len; i += 256) out[i] = src[rows[i]];
}
struct FilterV16 {
  unsigned long long lo, hi;
};

// blockIdx.x = output batch (exactly those of the kept rows), blockIdx.y = column
extern "C" __global__ void __launch_bounds__(256)
filter_gather_kernel(const FilterGatherJob* jobs, const uint32_t* src_rows, uint64_t kept, uint32_t B, uint32_t W) {
  __shared__ unsigned long long wsum[4];
  __shared__ unsigned long long carry_s;
  const FilterGatherJob j = jobs[blockIdx.y];
  const FilterCol& c = j.src;
  const uint64_t ob = blockIdx.x, first = ob * B;
  if (first >= kept) return;
  const uint32_t len = (uint32_t)(kept - first < B ? kept - first : B);
  const uint32_t* rows = src_rows + first;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // ---- validity and Boolean value bits, by ballot ----
  if (j.out_validity || c.kind == FKIND_BOOL) {
    for (uint32_t i0 = 0; i0 < len; i0 += 256) {
      const uint32_t i = i0 + threadIdx.x;
      const bool live = i < len;
      const uint64_t row = live ? rows[i] : 0;
      const uint64_t u = row / B;
      const uint32_t l = (uint32_t)(row % B);
      const unsigned long long lm = __ballot(live);
      if (j.out_validity) {
        const unsigned long long vm = __ballot(live && filter_valid(c, u, l, W));
        if (lane == 0 && lm) j.out_validity[ob * W + (i >> 6)] = vm;
      }
      if (c.kind == FKIND_BOOL) {
        const bool bit = live && ((reinterpret_cast<const unsigned long long*>(c.values)[u * W + (l >> 6)] >> (l & 63)) & 1);
        const unsigned long long bm = __ballot(bit);
        if (lane == 0 && lm) reinterpret_cast<unsigned long long*>(j.out_values)[ob * W + (i >> 6)] = bm;
      }
    }
  }
  if (c.kind == FKIND_BOOL) return;
  // ---- fixed-width values ----
  if (c.kind != FKIND_STRING) {
    uint8_t* out = j.out_values + first * c.width;
    switch (c.width) {
      case 1: filter_gather_fixed<uint8_t>(c.values, out, rows, len); break;
      case 2: filter_gather_fixed<uint16_t>(c.values, out, rows, len); break;
      case 4: filter_gather_fixed<uint32_t>(c.values, out, rows, len); break;
      case 8: filter_gather_fixed<unsigned long long>(c.values, out, rows, len); break;
      case 16: filter_gather_fixed<FilterV16>(c.values, out, rows, len); break;
      default: break;
    }
    return;
  }
  // ---- strings: lengths -> offsets of the batch (exclusive scan, restarting at 0) ----
  int32_t* ooff = j.out_offsets + ob * (B + 1);
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (uint32_t i0 = 0; i0 < len; i0 += 256) {
    const uint32_t i = i0 + threadIdx.x;
    unsigned long long n = 0;
    if (i < len) {
      const uint64_t row = rows[i];
      n = filter_str_len(c, row / B, (uint32_t)(row % B), B);
    }
    unsigned long long inc = n;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long y = (unsigned long long)__shfl_up((long long)inc, o);
      if (lane >= (uint32_t)o) inc += y;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned long long before = carry_s;
    for (uint32_t x = 0; x < wave; x++) before += wsum[x];
    if (i < len) ooff[i] = (int32_t)(uint32_t)(before + inc - n);
    __syncthreads();
    if (threadIdx.x == 255) carry_s = before + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) ooff[len] = (int32_t)(uint32_t)carry_s;
  // ---- ... and the bytes: a lane per short value, then a wavefront per long one ----
  uint8_t* dst0 = j.out_chars + j.out_char_base[ob];
  for (uint32_t i = threadIdx.x; i < len; i += 256) {
    const uint64_t row = rows[i];
    const uint64_t u = row / B;
    const int32_t* o = c.offsets + u * (B + 1) + (uint32_t)(row % B);
    const uint32_t a = (uint32_t)o[0], n = (uint32_t)o[1] - a;
    if (n == 0 || n > kFilterShortString) continue;
    const uint8_t* p = c.chars + c.char_base[u] + a;
    uint8_t* d = dst0 + (uint32_t)ooff[i];
    for (uint32_t x = 0; x < n; x++) d[x] = p[x];
  }
  for (uint32_t i = wave; i < len; i += 4) {
    const uint64_t row = rows[i];
    const uint64_t u = row / B;
    const int32_t* o = c.offsets + u * (B + 1) + (uint32_t)(row % B);
    const uint32_t a = (uint32_t)o[0], n = (uint32_t)o[1] - a;
    if (n <= kFilterShortString) continue;
    const uint8_t* p = c.chars + c.char_base[u] + a;
    uint8_t* d = dst0 + (uint32_t)ooff[i];
    for (uint32_t x = lane; x < n; x += 64) d[x] = p[x];
  }
}
