// orcgpu_decode_host.inc -- what a decode call plans on the host with plain arithmetic: the job types, the layout of the jobs
// (class order, block ranges, expansion groups: layout_jobs) and the dealing of root columns to lanes (deal_lanes).
//
// No HIP in this file and nothing of the context: tests/hostcheck/decode_host_check.cpp compiles it for the host, under
// AddressSanitizer, against transcriptions of the code blocks decode_lane and decode_staged_once held before.  The three device
// constants it needs are stated here; orcgpu.hip ties them to the device headers with a static_assert.
#include <algorithm>
#include <cstdint>
#include <vector>

namespace {

struct StagedStream;

constexpr uint32_t kJobBlockBytes = 512;   // RLE_BLK (device/rle_kernels.h)
constexpr uint32_t kJobTileBlocks = 1024;  // RLE_TILE
constexpr uint8_t kJobCodecByte = 2;       // CODEC_BYTE (device/rle_parse.h)

// Zstandard: sequences of a call from which on the FSE chains go one lane per block (zstd_lanes.h) instead of one wavefront per
// block: below it the call lasts as long as its longest chain either way (SF 3: 32 against 22 ms with the lanes forced on)
constexpr uint64_t kZstdLanesMinSequences = 40000000ull;

// ---- per-call plan ------------------------------------------------------------------------------
// (JC_PRESENT1 + d - 1: PRESENT streams of the fields of Structs / arms of Unions at depth d: they are as long as their parent has non-null rows)
// kMaxStructDepth classes of them: the reference recurses without a limit (array_decoder/mod.rs:464-505); here the depth is bounded
// by a number no schema reaches (the type tree of a file is walked recursively on the host: kMaxTypeDepth), and the PRESENT
// phase loops over the depths a call really has
constexpr int kMaxStructDepth = 256;
enum JobClass { JC_PRESENT = 0, JC_RLE2 = 1, JC_RLE1 = 2, JC_BYTE = 3, JC_PRESENT1 = 4, JC_COUNT = JC_PRESENT1 + kMaxStructDepth };

struct JobPlan {
  int cls;
  uint8_t codec, is_signed, nbits, out_bytes;
  const uint8_t* data;      // device pointer to the plain stream (may be assigned later)
  uint64_t data_scratch_off = ~0ull;  // when the plain stream lives in scratch (decompressed)
  uint64_t len_upper;       // upper bound of the plain length
  uint32_t len_idx, needed_idx, total_idx;
  uint64_t out_scratch_off = ~0ull;   // dense output in scratch ...
  uint64_t out_result_off = ~0ull;    // ... or directly in the result arena
  int result_index = 0;
  uint64_t expect_values;   // host estimate of values (for group sizing)
  // filled while laying out
  uint32_t block0 = 0, nblocks = 0, group0 = 0, ngroups = 0, group_size = 64;
  uint32_t skip_values = 0;            // of the stream's entry point: decoded in front of the output (RleJob::skip)
  const StagedStream* hint_src = nullptr;  // verified run starts, if the stream has any
  uint32_t chunk0 = 0;
  uint32_t uniform_idx = 0, uniform_value = 0;  // RleJob::uniform_idx / uniform_value (a Decimal column's scales)
  int stripe = 0, col = 0, role = 0;  // role: stream kind the job decodes
  int final_index = -1;
};

// ---- lay out jobs: class order, tile aligned block ranges, expansion groups ------------------------
struct JobLayout {
  std::vector<int> order;                  // the jobs in class order (stable): order[k] is the job with final_index k
  uint32_t cls_first[JC_COUNT + 1] = {0};  // final_index of a class's first job ([JC_COUNT]: the number of jobs)
  uint32_t cls_groups[JC_COUNT] = {0};     // expansion groups of a class
  uint32_t cls_tab0[JC_COUNT + 1] = {0};   // a class's first group in the call's group table (RleBlocks::group_job)
  uint64_t total_blocks = 0;               // of the tile aligned block ranges
  uint64_t call_blocks = 0;                // stream blocks of all jobs of the call (before their ranges are aligned)
  uint32_t n_tiles = 0;
  bool fits = true;                        // false: 2^32 blocks or more -- the call is refused, n_tiles and cls_tab0 are not set
};

constexpr uint64_t kGroupTarget = 6144;  // (measured 3072 .. 24576: the headline 35.7 - 35.9 ms at 3072 / 6144, 36.2 - 36.4 at 12288; C2 0.55 against 0.59 - 0.60)

JobLayout layout_jobs(std::vector<JobPlan>& jobs) {
  JobLayout L;
  L.order.resize(jobs.size());
  for (size_t i = 0; i < L.order.size(); i++) L.order[i] = (int)i;
  std::stable_sort(L.order.begin(), L.order.end(), [&](int a, int b) { return jobs[a].cls < jobs[b].cls; });
  for (const JobPlan& j : jobs) L.call_blocks += std::max<uint64_t>(1, (j.len_upper + kJobBlockBytes - 1) / kJobBlockBytes);
  int cur = 0;
  for (size_t k = 0; k < L.order.size(); k++) {
    JobPlan& j = jobs[L.order[k]];
    while (cur < j.cls) L.cls_first[++cur] = (uint32_t)k;
    j.final_index = (int)k;
    j.nblocks = (uint32_t)std::max<uint64_t>(1, (j.len_upper + kJobBlockBytes - 1) / kJobBlockBytes);
    j.block0 = (uint32_t)L.total_blocks;
    L.total_blocks += ((uint64_t)j.nblocks + kJobTileBlocks - 1) / kJobTileBlocks * kJobTileBlocks;
    // group size (blocks per wavefront of the expansion): bound the bytes one wavefront writes; keep enough wavefronts in flight --
    // over the CALL, not per stream: about kGroupTarget groups in all, and 64 or more of every stream --; a power of two, so that
    // 64 / g runs per block and trip use every lane.  (Round 5: nblocks / 512 per stream, whatever else the call held: lineitem's
    // dictionary-key streams -- 1500 - 2300 blocks a stripe -- got groups of 2 - 4 blocks, and the chain of run headers inside a
    // block, walked by the block's one lane, cost 16 - 32 hops per trip for a wavefront with 2 - 4 lanes at work.)
    double out_per_block = (double)j.expect_values * j.out_bytes / j.nblocks;
    uint32_t g = out_per_block > 0 ? (uint32_t)std::min<double>(64.0, std::max<double>(1.0, 131072.0 / out_per_block)) : 64;
    if (j.codec == kJobCodecByte) {
      // (byte RLE -- PRESENT bitmaps, Byte columns --: long runs, a block expands 8 - 60 times; more and smaller groups, as before:
      // C3's PRESENT expansion 0.16 ms with 512 groups a stream, 0.26 with the call-wide rule)
      g = std::min<uint32_t>(g, std::max<uint32_t>(1, j.nblocks / 512));
    } else {
      g = std::min<uint32_t>(g, std::max<uint32_t>(1, (uint32_t)(L.call_blocks / kGroupTarget)));
      g = std::min<uint32_t>(g, std::max<uint32_t>(1, j.nblocks / 64));
    }
    uint32_t p2 = 1;
    while (p2 * 2 <= g) p2 *= 2;
    j.group_size = p2;
    j.ngroups = (j.nblocks + p2 - 1) / p2;
    j.group0 = L.cls_groups[j.cls];
    L.cls_groups[j.cls] += j.ngroups;
  }
  while (cur < JC_COUNT) L.cls_first[++cur] = (uint32_t)L.order.size();
  L.fits = L.total_blocks < (1ull << 32);
  if (!L.fits) return L;
  L.n_tiles = (uint32_t)(L.total_blocks / kJobTileBlocks);
  for (int c = 0; c < JC_COUNT; c++) L.cls_tab0[c + 1] = L.cls_tab0[c] + L.cls_groups[c];
  return L;
}

// ---- lanes: whole columns, balanced by their staged bytes (longest first); a column that alone is a quarter of the
// call gets a lane to itself (its decompression is a serial chain per block: what runs beside it is free) -------------
// (a Struct and its fields stay on one lane: the fields' validity is built from the Struct's.  Columns are keyed by the id
// of the root column above them.)
struct LaneRoot {
  uint32_t column_id;  // of the root column
  uint64_t bytes;      // staged bytes of the streams of the root and everything below it, over all stripes of the call
  uint32_t max_nseq;   // sequences of the longest Zstandard block among those streams
};
struct LaneDeal {
  std::vector<int> lane_of;  // per root, in the order given
  int n_lanes = 1;
  int call_z = -1;  // the call's Zstandard path when the call is split over lanes (orcgpu_ctx::call_z_lanes)
};

// `seq_all`: Zstandard sequences of all streams of the call; `n_lanes`: lanes wanted (at most one per column); `forced`: by ORCGPU_LANES
LaneDeal deal_lanes(const std::vector<LaneRoot>& roots, uint64_t seq_all, int n_lanes, bool forced) {
  LaneDeal D;
  D.lane_of.assign(roots.size(), 0);
  D.n_lanes = n_lanes;
  if (n_lanes <= 1) return D;
  // longest first (equal weights: the lower column id)
  std::vector<size_t> w(roots.size());
  for (size_t k = 0; k < w.size(); k++) w[k] = k;
  std::sort(w.begin(), w.end(), [&](size_t a, size_t b) { return roots[a].bytes != roots[b].bytes ? roots[a].bytes > roots[b].bytes : roots[a].column_id < roots[b].column_id; });
  uint64_t total = 0;
  uint32_t mxmax = 0;
  for (const LaneRoot& r : roots) total += r.bytes, mxmax = std::max(mxmax, r.max_nseq);
  auto bytes = [&](size_t k) { return roots[w[k]].bytes; };
  auto mx = [&](size_t k) { return (uint64_t)roots[w[k]].max_nseq; };
  auto put = [&](size_t k, int lane, std::vector<uint64_t>& load) {
    D.lane_of[w[k]] = lane;
    load[lane] += bytes(k);
  };
  std::vector<uint64_t> load(n_lanes, 0);
  std::vector<bool> closed(n_lanes, false);
  for (size_t k = 0; k < w.size(); k++) {
    int best = -1;
    for (int l = 0; l < n_lanes; l++)
      if (!closed[l] && (best < 0 || load[l] < load[best])) best = l;
    if (best < 0) best = 0;
    put(k, best, load);
    if (k == 0 && w.size() > 1 && bytes(0) * 4 >= total) closed[best] = true;
  }
  // Zstandard: the entropy stage lasts as long as its longest block (a serial FSE chain, ~150 ns per sequence).  Columns whose
  // blocks come near the longest one of the call share lane 0; everything else -- its own entropy stage is short -- goes through
  // its whole pipeline on the other lanes meanwhile.
  // (one decision for the call: a lane whose own columns hold fewer sequences than the threshold took the other path -- SF 3: 32 against 22 ms)
  D.call_z = seq_all >= kZstdLanesMinSequences ? 1 : 0;
  std::vector<uint64_t> lload(n_lanes, 0);
  if (mxmax >= 4096 && n_lanes == 2 && seq_all >= kZstdLanesMinSequences) {
    // Table scale (the sequences go one lane per block, zstd_lanes.h): that kernel lasts as long as the call's longest chains and
    // leaves most of the machine idle meanwhile.  The columns with the longest chains share lane 0, the others are dealt out by
    // their staged bytes (largest first) -- lane 0 starting with a handicap for the wait -- so that the other lane's execution,
    // walk and finishing kernels run beside it and both lanes end together (SF 12.5: 69.8 -> 66.9 ms; the handicap a fifth of the staged bytes since the decimal finisher takes 4 ms instead of 7.4: 51.4 -> 48.4 ms).
    // per mille of the staged bytes.  (Round 6, twice in its first half: 0 .. 600 measured, 35.1 - 36.2 ms at every setting, no trend;
    // again at the round's last kernels -- the finishers of lane 0's Decimal columns 1.5 ms shorter --: 0 -> 33.1, 33.1; 200 -> 33.7, 33.9;
    // 300 -> 33.3, 33.5; 500 -> 33.6, 33.6; 700 -> 33.7, 34.1 ms: no head start any more)
    const uint64_t handicap = 0;
    lload[0] = total * handicap / 1000;
    for (size_t k = 0; k < w.size(); k++)
      if (mx(k) * 5 >= mxmax * 3ull) put(k, 0, lload);
    for (size_t k = 0; k < w.size(); k++)
      if (mx(k) * 5 < mxmax * 3ull) put(k, lload[1] < lload[0] ? 1 : 0, lload);
  } else if (mxmax >= 4096) {
    size_t heavy = 0;
    for (size_t k = 0; k < w.size(); k++) heavy += mx(k) * 2 >= mxmax;
    if (heavy == w.size() && !forced) D.n_lanes = n_lanes = 1;  // nothing light to run beside the heavy columns
    if (heavy < w.size())
      for (size_t k = 0; k < w.size(); k++) {
        if (mx(k) * 2 >= mxmax) {
          D.lane_of[w[k]] = 0;
        } else {
          int best = 1;
          for (int l = 2; l < n_lanes; l++)
            if (lload[l] < lload[best]) best = l;
          put(k, best, lload);
        }
      }
  }
  // lanes that got nothing are dropped
  for (int l = n_lanes - 1; l >= 1; l--) {
    bool any = false;
    for (int v : D.lane_of) any |= v == l;
    if (!any && l == D.n_lanes - 1) D.n_lanes--;
  }
  return D;
}

}  // namespace
