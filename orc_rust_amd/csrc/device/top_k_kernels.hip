// top_k_kernels.hip -- ORDER BY ... LIMIT k over the kept rows of a decoded stripe: a radix SELECT finds the k smallest rows under
// the sort keys without moving a row, a stable LSD radix SORT orders those at most k rows.  The semantics are those of
// include/orcgpu.h ("Top-k"); the key string -- the bytes whose unsigned order is that order -- is device/top_k_program.h's, and it
// is never materialised for the input rows: top_k_digit computes one byte of one row from the column, through the row access
// every kernel shares (filter_access.h).
//
// n_in input rows, n_words = ceil(n_in / 64) words of a plane; L = the key string's bytes; cap = min(k, n_in).
//
//   top_k_init_kernel          cand = the keep mask (none: every input row), win = 0, state.remaining = k.
//   per pass p = 0 .. L - 1, most significant byte first (the launch sequence is the host's, by the key kinds alone):
//     top_k_pass_kernel        over the words of `cand`: FIRST the bin pass p - 1 chose is applied -- a candidate whose byte p - 1 is
//                              below the bin enters `win`, one in the bin stays a candidate, one above leaves --, THEN byte p of the
//                              candidates left is counted, 256 bins in LDS a block -> hist[block][bin].
//     top_k_choose_kernel      one block: the bins summed over the blocks, a prefix sum over the 256 of them, the bin in which the
//                              running count crosses the remainder -> state.bin[p], and the remainder left for that bin.  When
//                              the bin holds exactly the remainder -- or, at pass 0, the candidates are no more than k -- nothing
//                              is left to decide: state.done.  Every later pass and choice is launched and leaves at once.
//   top_k_pass_kernel (p = L)  applies the last bin and counts nothing.
//   top_k_tie_count_kernel     the candidates left are tied on the whole key: their count per word, for enc_scan
//   top_k_final_kernel         a tied candidate whose rank among them -- the word's prefix count plus a popcount: ascending row order --
//                              is below the remainder wins.  final = win | those, and its popcount per word.
//   (enc_scan, filter_place_kernel: the winners' plane -> the row list, at most k rows in ascending input order)
//   per pass p = L - 1 .. 0, least significant byte first, over the row list:
//     top_k_sort_hist_kernel   a block per tile of kTopKSortTile winners: its rows per byte p -> hist[bin][block]
//     group_wide_scan_kernel   (agg_group_wide_kernels.hip, as it is) the exclusive prefix sum over [bin][block]
//     top_k_sort_scatter_kernel  a row's place: where its block's rows of its bin begin, plus those of its bin in the wavefronts in
//                              front of its own, plus those in the words of its wavefront in front of its own, plus its rank among
//                              the lanes of its word with its bin -- the scatter of group_wide_scatter_kernel, with bytes from
//                              top_k_digit and not from a key array.  Stable: equal keys keep ascending input-row order.
//   top_k_records_kernel       the winners' key strings, in sorted order, for the host's merge of the stripes
//   (filter_count_kernel, the one wait, filter_gather_kernel: as for the row filter)
//
// What may race: the bins' counts in LDS (integer adds; a sum does not depend on their order).  No atomic decides a value, a place
// or an order, and none is floating-point.  A word of `cand` / `win` is read and written by one wavefront only.
// Bounds: nothing read back from memory is trusted as an index.  A bin is 8 bits by construction (a byte); state.bin is compared,
// never indexed with.  A row of the list is used below n_src (the stripe's rows), a place below the winners' count, which is
// clamped to cap; an input row is below n_in because `cand` is masked to the live rows when it is made and only ever loses bits.
// LDS: pass 1 KiB, choose 1 KiB, sort histogram 1 KiB, scatter 4 KiB.
//
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): in front of each kernel.  No kernel uses scratch.
#pragma once
#include <stdint.h>

#include "agg_group_wide_kernels.hip"
#include "top_k_program.h"

// Byte b (0: the null byte) of key k's part of the key string of row r
__device__ __forceinline__ uint32_t top_k_digit(const TopKKey& k, const FilterCol* cols, const FilterRow& r, uint32_t W, uint32_t b) {
  const FilterCol c = cols[k.col];
  const bool valid = filter_valid(c, r.u, r.l, W);
  unsigned long long hi = 0, lo = 0;
  if (valid && b) {
    if (k.kind == TK_INT) lo = top_k_image_i64(filter_load_i64(c, r.row));
    else if (k.kind == TK_BOOL) lo = filter_load_bit(c, r.u, r.l, W) ? 1ull : 0ull;
    else if (k.kind == TK_FLOAT) lo = top_k_image_f64(filter_load_f64(c, r.row));
    else {
      filter_load_dec128(c, r.row, &lo, &hi);
      hi = top_k_image_dec_hi(hi);
    }
  }
  return top_k_key_byte(k, valid, hi, lo, b);
}

// The live rows of word w: bit l = input row w * 64 + l is below n_in
__device__ __forceinline__ unsigned long long top_k_live_word(uint64_t n_in, uint64_t w) {
  const uint64_t first = w * 64;
  if (first >= n_in) return 0;
  return n_in - first >= 64 ? ~0ull : (1ull << (n_in - first)) - 1ull;
}

// A thread per word.
// Resource usage (gfx950): 8 VGPRs, 17 SGPRs, no scratch, no spill, no LDS; occupancy 8 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
top_k_init_kernel(const unsigned long long* keep, uint64_t n_in, uint32_t k, unsigned long long* cand, unsigned long long* win, TopKState* st) {
  const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (w == 0) st->remaining = k;
  if (w >= (n_in + 63) / 64) return;
  const unsigned long long live = top_k_live_word(n_in, w);
  cand[w] = keep ? keep[w] & live : live;
  win[w] = 0;
}

// prev / prev_b: the key and byte of pass p - 1 (p = 0: unused); key / b: those of pass p (p = n_pass: unused, nothing is counted).
// hist: [block][256].
// Resource usage (gfx950): 26 VGPRs, 86 SGPRs, no scratch, no spill, 1024 bytes of LDS; occupancy 8 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
top_k_pass_kernel(TopKKey prev, uint32_t prev_b, TopKKey key, uint32_t b, uint32_t p, uint32_t n_pass, KeptRows rows, unsigned long long* cand,
                  unsigned long long* win, const TopKState* st, uint32_t* hist) {
  __shared__ uint32_t hist_s[256];
  const uint32_t done = st->done, last = st->last;
  const bool apply = p > 0 && !(done && last + 1 < p);  // (the bin of pass p - 1 has been chosen and not applied yet)
  const bool count = !done && p < n_pass;
  if (!apply && !count) return;  // (uniform over the grid: nothing is left to decide, and top_k_choose_kernel reads no bin count)
  const uint32_t bin = apply ? st->bin[p - 1] : 0;
  hist_s[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const FilterWords ws = filter_words(rows.n_in);
  for (uint64_t w = ws.first; w < ws.n; w += ws.stride) {
    unsigned long long m = cand[w];
    if (!m) continue;  // (uniform over the wavefront)
    const FilterRow r = filter_row(rows, w * 64 + lane);
    bool in = r.live && ((m >> lane) & 1);
    if (apply) {
      const uint32_t d = in ? top_k_digit(prev, rows.cols, r, rows.W, prev_b) : 0;
      const unsigned long long below = __ballot(in && d < bin), stay = __ballot(in && d == bin);
      if (lane == 0) {
        if (below) win[w] |= below;
        cand[w] = stay;
      }
      m = stay;
      in = (stay >> lane) & 1;
    }
    if (!count || !m) continue;
    const uint32_t d = in ? top_k_digit(key, rows.cols, r, rows.W, b) : 0;
    // (the upper bytes of a column are mostly one value: a word whose candidates all hold the same byte is one add)
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl((int)d, (int)__builtin_ctzll(m)));
    if (__ballot(in && d != d0) == 0) {
      if (lane == 0) atomicAdd(&hist_s[d0 & 255u], (uint32_t)__popcll(m));
    } else if (in) atomicAdd(&hist_s[d & 255u], 1u);
  }
  __syncthreads();
  if (count) hist[(uint64_t)blockIdx.x * 256 + threadIdx.x] = hist_s[threadIdx.x];
}

// <<<1, 256>>>: thread d takes bin d.
// Resource usage (gfx950): 11 VGPRs, 22 SGPRs, no scratch, no spill, 1024 bytes of LDS; occupancy 8 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
top_k_choose_kernel(uint32_t p, uint32_t n_blocks, const uint32_t* hist, TopKState* st) {
  __shared__ uint32_t sum_s[256];
  if (st->done) return;  // (uniform)
  const uint32_t d = threadIdx.x, rem = st->remaining;
  uint32_t c = 0;
  for (uint32_t blk = 0; blk < n_blocks; blk++) c += hist[(uint64_t)blk * 256 + d];
  sum_s[d] = c;
  __syncthreads();
  for (uint32_t o = 1; o < 256; o <<= 1) {
    const uint32_t v = d >= o ? sum_s[d - o] : 0;
    __syncthreads();
    sum_s[d] += v;
    __syncthreads();
  }
  const uint32_t incl = sum_s[d], excl = incl - c, total = sum_s[255];
  if (total <= rem) {  // fewer candidates than asked for (pass 0 alone can find that): every one of them wins
    if (d == 0) {
      if (p == 0) st->kept = total;
      st->bin[p] = kTopKEveryBin;
      st->remaining = rem - total;
      st->last = p;
      st->done = 1;
    }
    return;
  }
  if (d == 0 && p == 0) st->kept = total;
  if (excl < rem && rem <= incl) {  // exactly one bin: rem >= 1, the counts are not negative, total > rem
    st->bin[p] = d;
    st->remaining = rem - excl;
    st->last = p;
    st->done = c == rem - excl ? 1u : 0u;
  }
}

// A thread per word: cnt[w] = the candidates of word w.
// Resource usage (gfx950): 6 VGPRs, 14 SGPRs, no scratch, no spill, no LDS; occupancy 8 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
top_k_tie_count_kernel(const unsigned long long* cand, uint64_t n_words, uint32_t* cnt) {
  const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (w < n_words) cnt[w] = (uint32_t)__popcll(cand[w]);
}

// A thread per word.  woff: the exclusive prefix sums of top_k_tie_count_kernel's counts.  final_plane / cnt: the winners.
// Resource usage (gfx950): 10 VGPRs, 26 SGPRs, no scratch, no spill, no LDS; occupancy 8 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
top_k_final_kernel(const unsigned long long* cand, const unsigned long long* win, const unsigned long long* woff, const TopKState* st, uint64_t n_words,
                   unsigned long long* final_plane, uint32_t* cnt) {
  const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= n_words) return;
  const unsigned long long m = cand[w], before = woff[w], rem = st->remaining;
  unsigned long long take = 0;
  if (before < rem) {
    const unsigned long long room = rem - before;
    if (room >= (unsigned long long)__popcll(m)) take = m;
    else {
      unsigned long long t = m;
      for (unsigned long long i = 0; i < room; i++) {  // (the lowest `room` of its bits: fewer than 64 steps, in one word of the plane at most)
        const unsigned long long low = t & (0ull - t);
        take |= low;
        t ^= low;
      }
    }
  }
  const unsigned long long f = win[w] | take;
  final_plane[w] = f;
  cnt[w] = (uint32_t)__popcll(f);
}

// The rows a sort pass takes: the winners' count, never above cap = min(k, n_in)
__device__ __forceinline__ uint32_t top_k_winners(const unsigned long long* total, uint32_t cap) { return *total < cap ? (uint32_t)*total : cap; }
// Row e of the list, as the decode laid it out (a row past the stripe's: row 0, whose loads stay in bounds)
__device__ __forceinline__ FilterRow top_k_list_row(const uint32_t* list, uint64_t e, uint64_t n_src, uint32_t B) {
  const uint32_t row = list[e];
  return filter_row_of(row < n_src ? row : 0, B);
}

// hist: [bin][block], a block per tile of the list
// Resource usage (gfx950): 16 VGPRs, 47 SGPRs, no scratch, no spill, 1024 bytes of LDS; occupancy 8 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
top_k_sort_hist_kernel(TopKKey key, uint32_t b, const FilterCol* cols, uint32_t B, uint32_t W, uint64_t n_src, const uint32_t* rows_in,
                       const unsigned long long* total, uint32_t cap, uint32_t* hist) {
  __shared__ uint32_t hist_s[256];
  hist_s[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t n = top_k_winners(total, cap);
  for (uint32_t i = 0; i < kTopKSortTile / 256; i++) {
    const uint64_t e = (uint64_t)blockIdx.x * kTopKSortTile + i * 256 + threadIdx.x;
    if (e < n) atomicAdd(&hist_s[top_k_digit(key, cols, top_k_list_row(rows_in, e, n_src, B), W, b) & 255u], 1u);
  }
  __syncthreads();
  hist[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] = hist_s[threadIdx.x];
}

// hist: the exclusive sums over [bin][block].  at_s[v][d]: first the rows of bin d in wavefront v, then where wavefront v's next row
// of bin d goes.
// Resource usage (gfx950): 42 VGPRs, 61 SGPRs, no scratch, no spill, 4096 bytes of LDS; occupancy 8 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
top_k_sort_scatter_kernel(TopKKey key, uint32_t b, const FilterCol* cols, uint32_t B, uint32_t W, uint64_t n_src, const uint32_t* rows_in, uint32_t* rows_out,
                          const unsigned long long* total, uint32_t cap, const uint32_t* hist) {
  __shared__ uint32_t at_s[4][256];
  constexpr uint32_t kWords = kTopKSortTile / 256;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t v = 0; v < 4; v++) at_s[v][threadIdx.x] = 0;
  __syncthreads();
  const uint32_t n = top_k_winners(total, cap);
  const uint64_t e0 = (uint64_t)blockIdx.x * kTopKSortTile + (uint64_t)wave * (kTopKSortTile / 4) + lane;
  uint32_t row[kWords], dig[kWords];
#pragma unroll
  for (uint32_t i = 0; i < kWords; i++) {
    const uint64_t e = e0 + i * 64;
    row[i] = 0;
    dig[i] = 0;
    if (e < n) {
      row[i] = rows_in[e];
      dig[i] = top_k_digit(key, cols, top_k_list_row(rows_in, e, n_src, B), W, b) & 255u;
      atomicAdd(&at_s[wave][dig[i]], 1u);
    }
  }
  __syncthreads();
  {
    uint32_t at = hist[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x];  // thread d: bin d, the wavefronts in their order
    for (uint32_t v = 0; v < 4; v++) {
      const uint32_t c = at_s[v][threadIdx.x];
      at_s[v][threadIdx.x] = at;
      at += c;
    }
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (uint32_t i = 0; i < kWords; i++) {
    const bool has = e0 + i * 64 < n;
    const unsigned long long peers = wide_match_digit(dig[i], has);
    const uint32_t rank = (uint32_t)__popcll(peers & below);
    uint32_t pos = 0;
    if (has) pos = at_s[wave][dig[i]] + rank;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // (every lane has read the bin's place before one lane moves it)
    if (has && rank == 0) at_s[wave][dig[i]] += (uint32_t)__popcll(peers);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (has && pos < n) rows_out[pos] = row[i];
  }
}

// A thread per winner: recs[e * stride .. + keys.len) = the key string of row list[e] (stride >= keys.len; the rest is left alone)
// Resource usage (gfx950): 20 VGPRs, 33 SGPRs, no scratch, no spill, no LDS; occupancy 8 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
top_k_records_kernel(TopKKeys keys, const FilterCol* cols, uint32_t B, uint32_t W, uint64_t n_src, const uint32_t* list, const unsigned long long* total, uint32_t cap,
                     uint32_t stride, uint8_t* recs) {
  const uint32_t n = top_k_winners(total, cap);
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const FilterRow r = top_k_list_row(list, e, n_src, B);
  uint8_t* out = recs + e * stride;
  const uint32_t nk = keys.n < kTopKMaxKeys ? keys.n : kTopKMaxKeys;
  for (uint32_t q = 0; q < nk; q++) {
    const TopKKey k = keys.key[q];
    if (k.first + k.bytes > stride || k.bytes > 17) continue;  // (what the host never plans)
    for (uint32_t b = 0; b < k.bytes; b++) out[k.first + b] = (uint8_t)top_k_digit(k, cols, r, W, b);
  }
}
