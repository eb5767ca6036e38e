// agg_group_wide_kernels.hip -- GROUP BY past kGroupMax groups a result: the kept rows of a decoded stripe sorted by their group,
// every group's rows reduced as one segment.  Taken when the limit of groups in one result was set above kGroupMax
// (orcgpu_reader_set_group_limits, orcgpu_result_aggregate_groups_limit) and then for the whole call, however few groups the rows
// hold; its cost follows the rows, not the limit.  The semantics are those of include/orcgpu.h; the sibling for at most kGroupMax
// groups is agg_group_kernels.hip, whose key hash, key comparison, probing (group_assign_body) and key records (group_store_keys)
// are used here as they are, as are agg_row / agg_expr_row / agg_fold / agg_wave_fold / agg_store of agg_kernels.hip.
//
// n_in input rows in n_words = ceil(n_in / 64) words of the keep mask; a TILE is kGroupWideTile (2048) consecutive input rows or
// sorted pairs: 8 words for each of a block's 4 wavefronts, wavefront v taking words 8 v .. 8 v + 7 of the tile, in that order.
//
//   group_wide_assign_kernel    group_assign_body against a table of `slots` slots (the power of two >= 4 x the limit): plane[j] =
//                               the slot of kept row j, the slot's smallest row in first_inv.  GROUP_TOO_MANY at claim limit + 1.
//   group_wide_count_kernel     a block per tile: how many of its rows are kept, and how many are FIRST rows -- kept, and
//                               ~table[plane[j]].first_inv == j.
//   group_wide_scan_kernel      one block: an exclusive prefix sum, in place, over the blocks' counts.  The total of the first rows
//                               is n_groups (above the limit: GROUP_TOO_MANY), the total of the kept rows ctl->kept.
//   group_wide_number_kernel    a block per tile again: a first row's dense group number is the first rows in front of it -- the
//                               tile's offset plus a popcount over ballots --, so groups are numbered in first-appearance order by
//                               construction.  It writes slot_group[slot] and the group's GroupKeyRecords, and for every kept row
//                               its input row at the row's rank among the kept rows: the sort's input, in ascending row order.
//   group_wide_keys_kernel      a pair's key: the group number of its row, slot_group[plane[row]].
//   per pass of the sort -- LSD radix over (group, row) pairs, kGroupRadixBits (8) bits a pass, ceil(log2(limit) / 8) passes, so
//   the launch sequence is the host's choice by the limit and never the data's:
//     group_wide_hist_kernel    a block per tile: its pairs per digit -> hist[digit][block]
//     group_wide_scan_kernel    the exclusive prefix sum over [digit][block]: where a block's pairs of a digit begin
//     group_wide_scatter_kernel a block per tile: a pair's place is that beginning, plus the pairs of its digit in the wavefronts
//                               in front of its own (counted, then prefixed in wavefront order in LDS), plus those in the words of
//                               its wavefront in front of its own (a running count per digit in LDS, advanced word by word by one
//                               lane), plus its rank among the lanes of its word with its digit (a popcount over ballots).  No
//                               atomic decides a place: the sort is stable, and behind the last pass every group's rows stand
//                               together in ascending input-row order.
//   group_wide_segments_kernel  seg[g] = the first sorted pair of group g (a pair whose key differs from its predecessor's)
//   agg_group_wide_kernel, agg_group_wide_expr_kernel   grid (blocks, instructions): the reduction.  ONE WAVEFRONT folds one
//                               group (wavefront x of the grid takes groups x, x + wavefronts, ...) and stores the record
//                               (group, instruction) once with agg_store, into [group][instruction]: no partial, no final kernel.
//
// THE FOLD RULE.  Let r_0 < r_1 < ... < r_(c-1) be the kept input rows of a group, c >= 1.  Lane l (0 .. 63) starts from the empty
// accumulator and folds rows r_l, r_(l+64), r_(l+128), ... into it in that order (agg_row: a Float sum is acc = acc + value, from
// +0.0; a NULL value adds nothing); a lane l >= c keeps the empty accumulator.  Then agg_wave_fold: for o = 32, 16, 8, 4, 2, 1,
// lane l < o takes acc[l] = acc[l] (+) acc[l + o], the left operand in front.  Lane 0 holds the record.  The shape is a function
// of c alone -- not of the grid, the limit, the hash or the other groups -- so a Float sum is a function of the group's values in
// input-row order.  (c <= 64: one value a lane and the tree; c = 65 is the first count at which a lane adds serially.)
// COUNT_ROWS reads no row: it is c.
//
// What may race: the CAS and the Max of the table, the counts of group_wide_count_kernel and of the histograms (LDS integer adds),
// the flags.  None of them is a value, an order or a place.  No floating-point atomic.
// Bounds: a refused or overfull table leaves GROUP_TOO_MANY, final behind the first scan; every later kernel leaves at once under
// it.  Beyond that nothing read back from memory is trusted as an index: a slot is used below `slots`, a group below `cap` (the
// records' capacity: min(limit, n_in)), a row below n_in, a place below the pair count, which is clamped to n_in; a digit is 8 bits.
// LDS: the count kernel 8 bytes, the number kernel 256, the scan 4 KiB, the histogram 1 KiB, the scatter 4 KiB; the reduction none.
//
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): in front of each kernel.  No kernel uses scratch.
#pragma once
#include <stdint.h>

#include "agg_group_kernels.hip"

constexpr uint32_t kWideWords = kGroupWideTile / 256;  // words of a tile a wavefront takes: 8
static_assert(kGroupWideTile == 256 * kWideWords && kGroupRadixBits == 8, "a tile is 4 wavefronts x 8 words; a digit is a byte");

// Resource usage (gfx950): 65 VGPRs, 106 SGPRs (2 spilled to VGPR lanes), no scratch, no VGPR spill, no LDS; occupancy 7 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
group_wide_assign_kernel(GroupKeys keys, KeptRows rows, GroupSlot* table, uint32_t slots, uint32_t max_groups, GroupControl* ctl, uint32_t* plane) {
  group_assign_body(keys, rows, table, slots, max_groups, ctl, plane);
}

// Word q (0 .. 31) of the block's tile: which of its lanes hold a kept row, and which a group's first row
struct WideWord {
  unsigned long long kept, first;
};
__device__ __forceinline__ WideWord wide_word(const KeptRows& rows, const GroupSlot* table, uint32_t slots, const uint32_t* plane, uint32_t q, uint32_t* slot_out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t w = (uint64_t)blockIdx.x * (kGroupWideTile / 64) + q;
  *slot_out = kGroupNoSlot;
  if (w >= (rows.n_in + 63) / 64) return {0, 0};  // (uniform over the wavefront)
  const unsigned long long m = agg_keep_word(rows, w);
  if (!m) return {0, 0};  // (the plane holds nothing for a word without a kept row)
  const uint64_t j = w * 64 + lane;
  const bool kept = ((m >> lane) & 1) && j < rows.n_in;
  bool first = false;
  if (kept) {
    const uint32_t slot = plane[j];
    if (slot < slots) {
      *slot_out = slot;
      first = ~table[slot].first_inv == j;
    }
  }
  return {__ballot(kept), __ballot(first)};
}

// blk_first / blk_kept: [block], a block per tile
// Resource usage (gfx950): 25 VGPRs, 40 SGPRs, no scratch, no spill, 8 bytes of LDS; occupancy 8 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
group_wide_count_kernel(KeptRows rows, const GroupSlot* table, uint32_t slots, const uint32_t* plane, uint32_t* blk_first, uint32_t* blk_kept) {
  __shared__ uint32_t cnt_s[2];
  if (threadIdx.x < 2) cnt_s[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t first = 0, kept = 0, slot;
  for (uint32_t i = 0; i < kWideWords; i++) {
    const WideWord ww = wide_word(rows, table, slots, plane, wave * kWideWords + i, &slot);
    kept += (uint32_t)__popcll(ww.kept);
    first += (uint32_t)__popcll(ww.first);
  }
  if (lane == 0) {
    atomicAdd(&cnt_s[0], first);
    atomicAdd(&cnt_s[1], kept);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    blk_first[blockIdx.x] = cnt_s[0];
    blk_kept[blockIdx.x] = cnt_s[1];
  }
}

// <<<1, 1024>>>: data[0 .. n) -> its exclusive prefix sums, in place; thread t takes a run of ceil(n / 1024) entries.  total_out
// (may be null) gets the sum; a sum above `limit` (0: none) sets GROUP_TOO_MANY in *flags.
// Resource usage (gfx950): 14 VGPRs, 20 SGPRs, no scratch, no spill, 4096 bytes of LDS; occupancy 8 waves / SIMD.
extern "C" __global__ void __launch_bounds__(1024)
group_wide_scan_kernel(uint32_t* data, uint32_t n, uint32_t* total_out, uint32_t limit, uint32_t* flags) {
  __shared__ uint32_t part_s[1024];
  const uint32_t t = threadIdx.x, per = (n + 1023) / 1024;
  const uint64_t lo64 = (uint64_t)t * per;
  const uint32_t lo = lo64 < n ? (uint32_t)lo64 : n, hi = n - lo < per ? n : lo + per;
  uint32_t sum = 0;
  for (uint32_t k = lo; k < hi; k++) sum += data[k];
  part_s[t] = sum;
  __syncthreads();
  for (uint32_t o = 1; o < 1024; o <<= 1) {
    const uint32_t v = t >= o ? part_s[t - o] : 0;
    __syncthreads();
    part_s[t] += v;
    __syncthreads();
  }
  uint32_t run = part_s[t] - sum;
  for (uint32_t k = lo; k < hi; k++) {
    const uint32_t v = data[k];
    data[k] = run;
    run += v;
  }
  if (t == 1023 && total_out) {
    *total_out = part_s[1023];
    if (limit && part_s[1023] > limit) atomicOr(flags, (uint32_t)GROUP_TOO_MANY);
  }
}

// blk_first / blk_kept: the exclusive sums.  order_rows[p] = the input row of the p-th kept row; slot_group[slot] = the group of a
// claimed slot; key_recs: [group][key], `cap` groups.
// Resource usage (gfx950): 106 VGPRs (the eight words' ballots and slots are kept over the barrier), 62 SGPRs, no scratch, no spill,
// 256 bytes of LDS; occupancy 4 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
group_wide_number_kernel(GroupKeys keys, KeptRows rows, const GroupSlot* table, uint32_t slots, uint32_t cap, const uint32_t* plane, const uint32_t* blk_first,
                         const uint32_t* blk_kept, GroupControl* ctl, uint32_t* slot_group, GroupKeyRecord* key_recs, uint32_t* order_rows) {
  __shared__ uint32_t first_s[kGroupWideTile / 64], kept_s[kGroupWideTile / 64];
  if (ctl->flags & GROUP_TOO_MANY) return;  // (uniform: the whole grid leaves)
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  WideWord ww[kWideWords];
  uint32_t slot[kWideWords];
#pragma unroll
  for (uint32_t i = 0; i < kWideWords; i++) {
    ww[i] = wide_word(rows, table, slots, plane, wave * kWideWords + i, &slot[i]);
    if (lane == 0) {
      first_s[wave * kWideWords + i] = (uint32_t)__popcll(ww[i].first);
      kept_s[wave * kWideWords + i] = (uint32_t)__popcll(ww[i].kept);
    }
  }
  __syncthreads();
  uint32_t g0 = blk_first[blockIdx.x], p0 = blk_kept[blockIdx.x];
  for (uint32_t q = 0; q < wave * kWideWords; q++) {  // the words of the wavefronts in front of this one
    g0 += first_s[q];
    p0 += kept_s[q];
  }
#pragma unroll
  for (uint32_t i = 0; i < kWideWords; i++) {
    const uint64_t j = ((uint64_t)blockIdx.x * (kGroupWideTile / 64) + wave * kWideWords + i) * 64 + lane;
    if ((ww[i].kept >> lane) & 1) {
      const uint32_t p = p0 + (uint32_t)__popcll(ww[i].kept & below);
      if (p < rows.n_in) order_rows[p] = (uint32_t)j;
    }
    if ((ww[i].first >> lane) & 1) {
      const uint32_t g = g0 + (uint32_t)__popcll(ww[i].first & below);
      if (g < cap && slot[i] < slots) {
        slot_group[slot[i]] = g;
        group_store_keys(keys, rows, j, g, ctl, key_recs);
      }
    }
    g0 += (uint32_t)__popcll(ww[i].first);
    p0 += (uint32_t)__popcll(ww[i].kept);
  }
}

// The pairs of a call: the kept rows, never more than the input rows; none under GROUP_TOO_MANY
__device__ __forceinline__ uint32_t wide_pairs(const GroupControl* ctl, uint64_t n_in) {
  if (ctl->flags & GROUP_TOO_MANY) return 0;
  return ctl->kept < n_in ? ctl->kept : (uint32_t)n_in;
}

// order_keys[p] = the group of input row order_rows[p] (grid-stride over the pairs)
// Resource usage (gfx950): 8 VGPRs, 28 SGPRs, no scratch, no spill, no LDS; occupancy 8 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
group_wide_keys_kernel(const uint32_t* plane, const uint32_t* slot_group, uint32_t slots, uint32_t cap, uint64_t n_in, const GroupControl* ctl,
                       const uint32_t* order_rows, uint32_t* order_keys) {
  const uint32_t n = wide_pairs(ctl, n_in);
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256) {
    const uint32_t j = order_rows[p];
    const uint32_t slot = j < n_in ? plane[j] : kGroupNoSlot;
    const uint32_t g = slot < slots ? slot_group[slot] : 0;
    order_keys[p] = g < cap ? g : 0;
  }
}

// hist: [digit][block], a block per tile of pairs
// Resource usage (gfx950): 8 VGPRs, 20 SGPRs, no scratch, no spill, 1024 bytes of LDS; occupancy 8 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
group_wide_hist_kernel(const uint32_t* keys_in, uint32_t shift, uint64_t n_in, const GroupControl* ctl, uint32_t* hist) {
  __shared__ uint32_t hist_s[256];
  hist_s[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t n = wide_pairs(ctl, n_in);
  for (uint32_t i = 0; i < kWideWords; i++) {
    const uint64_t e = (uint64_t)blockIdx.x * kGroupWideTile + i * 256 + threadIdx.x;
    if (e < n) atomicAdd(&hist_s[(keys_in[e] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x] = hist_s[threadIdx.x];
}

// The lanes of the wavefront that hold a pair with this lane's digit (a lane without a pair: unused)
__device__ __forceinline__ unsigned long long wide_match_digit(uint32_t d, bool has) {
  unsigned long long peers = __ballot(has);
#pragma unroll
  for (uint32_t b = 0; b < kGroupRadixBits; b++) {
    const unsigned long long m = __ballot(has && ((d >> b) & 1));
    peers &= ((d >> b) & 1) ? m : ~m;
  }
  return peers;
}

// hist: the exclusive sums over [digit][block].  at_s[v][d]: first the pairs of digit d in wavefront v, then where wavefront v's
// next pair of digit d goes.
// Resource usage (gfx950): 16 VGPRs, 37 SGPRs, no scratch, no spill, 4096 bytes of LDS; occupancy 8 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
group_wide_scatter_kernel(const uint32_t* keys_in, const uint32_t* rows_in, uint32_t* keys_out, uint32_t* rows_out, uint32_t shift, uint64_t n_in,
                          const GroupControl* ctl, const uint32_t* hist) {
  __shared__ uint32_t at_s[4][256];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint32_t v = 0; v < 4; v++) at_s[v][threadIdx.x] = 0;
  __syncthreads();
  const uint32_t n = wide_pairs(ctl, n_in);
  const uint64_t e0 = (uint64_t)blockIdx.x * kGroupWideTile + (uint64_t)wave * (kGroupWideTile / 4) + lane;
  for (uint32_t i = 0; i < kWideWords; i++) {
    const uint64_t e = e0 + i * 64;
    if (e < n) atomicAdd(&at_s[wave][(keys_in[e] >> shift) & 255u], 1u);
  }
  __syncthreads();
  {
    uint32_t at = hist[(uint64_t)threadIdx.x * gridDim.x + blockIdx.x];  // thread d: digit d, the wavefronts in their order
    for (uint32_t v = 0; v < 4; v++) {
      const uint32_t c = at_s[v][threadIdx.x];
      at_s[v][threadIdx.x] = at;
      at += c;
    }
  }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  for (uint32_t i = 0; i < kWideWords; i++) {
    const uint64_t e = e0 + i * 64;
    const bool has = e < n;
    const uint32_t key = has ? keys_in[e] : 0, row = has ? rows_in[e] : 0, d = (key >> shift) & 255u;
    const unsigned long long peers = wide_match_digit(d, has);
    const uint32_t rank = (uint32_t)__popcll(peers & below);
    uint32_t pos = 0;
    if (has) pos = at_s[wave][d] + rank;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // (every lane has read the digit's place before one lane moves it)
    if (has && rank == 0) at_s[wave][d] += (uint32_t)__popcll(peers);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    if (has && pos < n) {
      keys_out[pos] = key;
      rows_out[pos] = row;
    }
  }
}

// seg: [cap]; the groups 0 .. n_groups - 1 each hold a pair, so each gets its start
// Resource usage (gfx950): 8 VGPRs, 26 SGPRs, no scratch, no spill, no LDS; occupancy 8 waves / SIMD.
extern "C" __global__ void __launch_bounds__(256)
group_wide_segments_kernel(const uint32_t* keys, uint32_t cap, uint64_t n_in, const GroupControl* ctl, uint32_t* seg) {
  const uint32_t n = wide_pairs(ctl, n_in);
  for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (uint64_t)gridDim.x * 256) {
    const uint32_t k = keys[p];
    if (k < cap && (p == 0 || keys[p - 1] != k)) seg[k] = (uint32_t)p;
  }
}

// out: [group][instruction], n_insn = gridDim.y records a group.  The fold rule of the head comment.
// Resource usage (gfx950): agg_group_wide_kernel 46 VGPRs, 102 SGPRs; agg_group_wide_expr_kernel 76 VGPRs, 106 SGPRs; both no scratch,
// no spill, no LDS: occupancy 7 waves / SIMD for the plain kernel, by its scalar registers -- the condition's plane (a pointer and
// the count of planes beside the rows) took it from 94 past the 100 that eight waves allow -- and 6 for the
// expression kernel, by its vector registers: seven waves allow 72.  agg_group_wide_expr_div_kernel, the
// expression kernel with the divide, which only a list that holds a division runs: 82 VGPRs, 106 SGPRs, no scratch, 5 waves (6o).
// A row whose instruction has a condition (AggInsn::cond) and does not pass it is a lane step that adds nothing: start, end, c and
// every row's lane stay those of the fold rule.  COUNT_ROWS under a condition counts the passing rows, lane by lane.
// (The body of two kernels, as agg_group_partial_body is: EXPR = false takes the plain kinds, EXPR = true the AK_EXPR_* rows of grid.y;
// DIV: the interpreter with the divide, agg_group_wide_expr_div_kernel, launched in its place when a program holds a division.)
template <bool EXPR, bool DIV = false, bool COND = false, bool CONV = false>
__device__ __forceinline__ void agg_group_wide_body(const AggInsn* insns, const AggExprOp* ops, const KeptRows& rows, const uint32_t* order_rows, const uint32_t* seg,
                                                    const GroupControl* ctl, uint32_t cap, AggPartial* out) {
  const FilterCol* const cols = rows.cols;
  const uint64_t n_in = rows.n_in;
  const uint32_t W = rows.W;
  if (ctl->flags & GROUP_TOO_MANY) return;  // (uniform: the whole grid leaves)
  const uint32_t n_groups = ctl->n_groups < cap ? ctl->n_groups : cap, n = wide_pairs(ctl, n_in);
  const AggInsn in = insns[blockIdx.y];
  if (agg_is_expr(in.kind) != EXPR) return;  // (uniform over the block)
  const uint32_t kind = EXPR ? in.kind : in.kind < AK_N ? in.kind : AK_COUNT_ROWS;
  const bool is_max = in.is_max != 0;
  const FilterCol c = cols[EXPR ? 0 : in.col], c2 = cols[EXPR ? 0 : in.col2];  // (EXPR: col / col2 are no column indexes; unused)
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bool blocked;
  const unsigned long long* const cond = agg_cond_plane(rows, in.cond, &blocked);
  if (blocked) return;  // (uniform over the block; the host has refused such a plan before any launch)
  for (uint64_t g = (uint64_t)blockIdx.x * 4 + wave; g < n_groups; g += (uint64_t)gridDim.x * 4) {
    const uint32_t start = seg[g], end = g + 1 < n_groups ? seg[g + 1] : n;
    AggAcc a = {0, 0, 0, 0.0, 0, 0};
    if (start <= end && end <= n) {  // (what the sort leaves; anything else folds to the empty record)
      if (!EXPR && kind == AK_COUNT_ROWS && !cond) {
        if (lane == 0) a.w0 = end - start;
      } else {
        for (uint32_t p = start + lane; p < end; p += 64) {
          const uint32_t j = order_rows[p];
          if (j >= n_in || !agg_row_passes(cond, j)) continue;  // (a row that does not pass: a lane step that adds nothing)
          if (!EXPR && kind == AK_COUNT_ROWS) {
            a.w0++;
            continue;
          }
          if constexpr (EXPR) agg_expr_row<DIV, COND, CONV>(kind, ops + in.col, in.col2, cols, filter_row(rows, j), W, a);
          else agg_row(kind, is_max, in, c, c2, filter_row(rows, j), W, a);
        }
        agg_wave_fold(kind, is_max, a);
      }
    }
    if (lane == 0) agg_store(out + g * gridDim.y + blockIdx.y, a);
  }
}
extern "C" __global__ void __launch_bounds__(256)
agg_group_wide_kernel(const AggInsn* insns, KeptRows rows, const uint32_t* order_rows, const uint32_t* seg, const GroupControl* ctl, uint32_t cap, AggPartial* out) {
  agg_group_wide_body<false>(insns, nullptr, rows, order_rows, seg, ctl, cap, out);
}
extern "C" __global__ void __launch_bounds__(256)
agg_group_wide_expr_kernel(const AggInsn* insns, const AggExprOp* ops, KeptRows rows, const uint32_t* order_rows, const uint32_t* seg, const GroupControl* ctl,
                           uint32_t cap, AggPartial* out) {
  agg_group_wide_body<true>(insns, ops, rows, order_rows, seg, ctl, cap, out);
}
extern "C" __global__ void __launch_bounds__(256)
agg_group_wide_expr_div_kernel(const AggInsn* insns, const AggExprOp* ops, KeptRows rows, const uint32_t* order_rows, const uint32_t* seg, const GroupControl* ctl,
                               uint32_t cap, AggPartial* out) {
  agg_group_wide_body<true, true>(insns, ops, rows, order_rows, seg, ctl, cap, out);
}
// (the interpreter with the divide and the conditionals: launched when a program of the list holds a conditional op)
extern "C" __global__ void __launch_bounds__(256)
agg_group_wide_expr_cond_kernel(const AggInsn* insns, const AggExprOp* ops, KeptRows rows, const uint32_t* order_rows, const uint32_t* seg, const GroupControl* ctl,
                                uint32_t cap, AggPartial* out) {
  agg_group_wide_body<true, true, true>(insns, ops, rows, order_rows, seg, ctl, cap, out);
}
// (the mixed interpreter: launched when a program of the list holds a conversion)
extern "C" __global__ void __launch_bounds__(256)
agg_group_wide_expr_conv_kernel(const AggInsn* insns, const AggExprOp* ops, KeptRows rows, const uint32_t* order_rows, const uint32_t* seg, const GroupControl* ctl,
                                uint32_t cap, AggPartial* out) {
  agg_group_wide_body<true, true, true, true>(insns, ops, rows, order_rows, seg, ctl, cap, out);
}
