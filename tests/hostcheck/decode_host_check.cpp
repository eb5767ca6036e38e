// decode_host_check.cpp -- the decode call's host planning (orc_rust_amd/csrc/orcgpu_decode_host.inc, the very text liborcgpu.so is
// built from) under AddressSanitizer + UBSan, on the CPU (TEST INFRASTRUCTURE).  layout_jobs and deal_lanes are compared, field by
// field, with `reference_layout` and `reference_lanes`: transcriptions of the two code blocks decode_lane and decode_staged_once
// held before the planning had functions of its own (what those blocks gathered from the staged stripes is handed to them).
// Seeded random inputs, then the edge cases by hand, each with the result it must give.
// Prints one line per case; exit code 0 when every case agreed; a sanitizer report aborts with its own exit code.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../orc_rust_amd/csrc/orcgpu_decode_host.inc"

#define RLE_BLK 512u
#define RLE_TILE 1024u
enum : int { CODEC_RLE2 = 0, CODEC_RLE1 = 1, CODEC_BYTE = 2 };
static inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// ---- the reference: the job layout as decode_lane computed it ----------------------------------------------------------------------
struct RefLayout {
  std::vector<int> order;
  uint32_t cls_first[JC_COUNT + 1] = {0}, cls_groups[JC_COUNT] = {0}, cls_tab0[JC_COUNT + 1] = {0};
  uint64_t total_blocks = 0, call_blocks = 0;
  uint32_t n_tiles = 0;
  bool refused = false;
};
static RefLayout reference_layout(std::vector<JobPlan>& jobs) {
  RefLayout R;
  std::vector<int> order(jobs.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return jobs[a].cls < jobs[b].cls; });
  uint32_t cls_first[JC_COUNT + 1] = {0}, cls_groups[JC_COUNT] = {0};
  uint64_t total_blocks = 0;
  uint64_t call_blocks = 0;
  for (const JobPlan& j : jobs) call_blocks += std::max<uint64_t>(1, (j.len_upper + RLE_BLK - 1) / RLE_BLK);
  constexpr uint64_t kGroupTarget = 6144;
  {
    int cur = 0;
    for (size_t k = 0; k < order.size(); k++) {
      JobPlan& j = jobs[order[k]];
      while (cur < j.cls) cls_first[++cur] = (uint32_t)k;
      j.final_index = (int)k;
      j.nblocks = (uint32_t)std::max<uint64_t>(1, (j.len_upper + RLE_BLK - 1) / RLE_BLK);
      j.block0 = (uint32_t)total_blocks;
      total_blocks += align_up(j.nblocks, RLE_TILE);
      double out_per_block = (double)j.expect_values * j.out_bytes / j.nblocks;
      uint32_t g = out_per_block > 0 ? (uint32_t)std::min<double>(64.0, std::max<double>(1.0, 131072.0 / out_per_block)) : 64;
      if (j.codec == CODEC_BYTE) {
        g = std::min<uint32_t>(g, std::max<uint32_t>(1, j.nblocks / 512));
      } else {
        g = std::min<uint32_t>(g, std::max<uint32_t>(1, (uint32_t)(call_blocks / kGroupTarget)));
        g = std::min<uint32_t>(g, std::max<uint32_t>(1, j.nblocks / 64));
      }
      {
        uint32_t p2 = 1;
        while (p2 * 2 <= g) p2 *= 2;
        g = p2;
      }
      j.group_size = g;
      j.ngroups = (j.nblocks + g - 1) / g;
      j.group0 = cls_groups[j.cls];
      cls_groups[j.cls] += j.ngroups;
    }
    while (cur < JC_COUNT) cls_first[++cur] = (uint32_t)order.size();
  }
  R.order = order;
  for (int c = 0; c <= JC_COUNT; c++) R.cls_first[c] = cls_first[c];
  for (int c = 0; c < JC_COUNT; c++) R.cls_groups[c] = cls_groups[c];
  R.total_blocks = total_blocks;
  R.call_blocks = call_blocks;
  if (total_blocks >= (1ull << 32)) {
    R.refused = true;
    return R;
  }
  R.n_tiles = (uint32_t)(total_blocks / RLE_TILE);
  uint32_t cls_tab0[JC_COUNT + 1] = {0};
  for (int c = 0; c < JC_COUNT; c++) cls_tab0[c + 1] = cls_tab0[c] + cls_groups[c];
  for (int c = 0; c <= JC_COUNT; c++) R.cls_tab0[c] = cls_tab0[c];
  return R;
}

// ---- the reference: the lanes as decode_staged_once dealt them (w and mx: what it gathered from the stripes) --------------------------
struct RefLanes {
  std::vector<std::pair<uint64_t, uint32_t>> w;  // sorted
  std::vector<int> lane_of;                      // per entry of w
  int n_lanes = 1, call_z = -1;
};
static RefLanes reference_lanes(const std::vector<LaneRoot>& roots, uint64_t seq_all, int n_lanes, bool forced_lanes) {
  RefLanes R;
  R.n_lanes = n_lanes;
  const bool auto_lanes = !forced_lanes && n_lanes > 1;
  int call_z = -1;
  if (n_lanes > 1) {
    std::vector<std::pair<uint64_t, uint32_t>> w;  // (bytes, column id)
    uint64_t total = 0;
    for (auto& r : roots) {
      w.push_back({r.bytes, r.column_id});
      total += r.bytes;
    }
    std::sort(w.begin(), w.end(), [](auto& a, auto& b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
    std::vector<uint64_t> load(n_lanes, 0);
    std::vector<int> lane_of(w.size(), 0);
    std::vector<bool> closed(n_lanes, false);
    for (size_t k = 0; k < w.size(); k++) {
      int best = -1;
      for (int l = 0; l < n_lanes; l++)
        if (!closed[l] && (best < 0 || load[l] < load[best])) best = l;
      if (best < 0) best = 0;
      lane_of[k] = best;
      load[best] += w[k].first;
      if (k == 0 && w.size() > 1 && w[0].first * 4 >= total && n_lanes > 1) closed[best] = true;
    }
    {
      std::vector<uint32_t> mx(w.size(), 0);
      uint32_t mxmax = 0;
      for (auto& r : roots) {
        size_t k = 0;
        for (; k < w.size(); k++)
          if (w[k].second == r.column_id) break;
        if (k == w.size()) continue;
        mx[k] = std::max(mx[k], r.max_nseq);
        mxmax = std::max(mxmax, mx[k]);
      }
      const uint64_t lanes_min = 40000000ull;
      call_z = seq_all >= lanes_min ? 1 : 0;
      if (mxmax >= 4096 && n_lanes == 2 && seq_all >= lanes_min) {
        std::vector<uint64_t> lload(n_lanes, 0);
        const uint64_t handicap = 0;
        lload[0] = total * handicap / 1000;
        for (size_t k = 0; k < w.size(); k++)
          if (mx[k] * 5ull >= mxmax * 3ull) {
            lane_of[k] = 0;
            lload[0] += w[k].first;
          }
        for (size_t k = 0; k < w.size(); k++)
          if (mx[k] * 5ull < mxmax * 3ull) {
            const int best = lload[1] < lload[0] ? 1 : 0;
            lane_of[k] = best;
            lload[best] += w[k].first;
          }
      } else if (mxmax >= 4096) {
        std::vector<uint64_t> lload(n_lanes, 0);
        size_t heavy = 0;
        for (size_t k = 0; k < w.size(); k++) heavy += mx[k] * 2ull >= mxmax;
        if (heavy == w.size() && auto_lanes) n_lanes = 1;  // nothing light to run beside the heavy columns
        if (heavy < w.size())
          for (size_t k = 0; k < w.size(); k++) {
            if (mx[k] * 2ull >= mxmax) {
              lane_of[k] = 0;
            } else {
              int best = 1;
              for (int l = 2; l < n_lanes; l++)
                if (lload[l] < lload[best]) best = l;
              lane_of[k] = best;
              lload[best] += w[k].first;
            }
          }
      }
    }
    // lanes that got nothing are dropped (a lane's mask is empty when no root is on it: every root has a column)
    for (int l = n_lanes - 1; l >= 1; l--) {
      bool any = false;
      for (int v : lane_of) any |= v == l;
      if (!any && l == n_lanes - 1) n_lanes--;
    }
    R.w = w;
    R.lane_of = lane_of;
  }
  R.n_lanes = n_lanes;
  R.call_z = call_z;
  return R;
}

// ---- comparing -----------------------------------------------------------------------------------------------------------------------
static int g_bad = 0, g_cases = 0;
#define CHECK(cond, ...)                   \
  do {                                     \
    if (!(cond)) {                         \
      if (g_bad++ < 30) {                  \
        printf("  MISMATCH %s: ", what);   \
        printf(__VA_ARGS__);               \
        printf("\n");                      \
      }                                    \
    }                                      \
  } while (0)

static JobPlan job(int cls, int codec, uint64_t len_upper, uint64_t expect_values, int out_bytes) {
  JobPlan j{};
  j.cls = cls;
  j.codec = (uint8_t)codec;
  j.out_bytes = (uint8_t)out_bytes;
  j.len_upper = len_upper;
  j.expect_values = expect_values;
  j.group_size = 64;
  j.final_index = -1;
  return j;
}

// layout_jobs against the reference, and what holds of every layout
static JobLayout check_layout(const char* what, std::vector<JobPlan>& jobs) {
  std::vector<JobPlan> rj = jobs;
  const RefLayout R = reference_layout(rj);
  const JobLayout L = layout_jobs(jobs);
  CHECK(L.order == R.order, "order");
  CHECK(L.total_blocks == R.total_blocks, "total_blocks %llu != %llu", (unsigned long long)L.total_blocks, (unsigned long long)R.total_blocks);
  CHECK(L.call_blocks == R.call_blocks, "call_blocks %llu != %llu", (unsigned long long)L.call_blocks, (unsigned long long)R.call_blocks);
  CHECK(L.fits == !R.refused, "fits %d, refused %d", (int)L.fits, (int)R.refused);
  for (int c = 0; c <= JC_COUNT; c++) CHECK(L.cls_first[c] == R.cls_first[c], "cls_first[%d] %u != %u", c, L.cls_first[c], R.cls_first[c]);
  for (int c = 0; c < JC_COUNT; c++) CHECK(L.cls_groups[c] == R.cls_groups[c], "cls_groups[%d] %u != %u", c, L.cls_groups[c], R.cls_groups[c]);
  if (L.fits) {
    CHECK(L.n_tiles == R.n_tiles, "n_tiles %u != %u", L.n_tiles, R.n_tiles);
    for (int c = 0; c <= JC_COUNT; c++) CHECK(L.cls_tab0[c] == R.cls_tab0[c], "cls_tab0[%d] %u != %u", c, L.cls_tab0[c], R.cls_tab0[c]);
  }
  for (size_t k = 0; k < jobs.size(); k++) {
    const JobPlan &a = jobs[k], &b = rj[k];
    CHECK(a.final_index == b.final_index && a.nblocks == b.nblocks && a.block0 == b.block0 && a.group_size == b.group_size && a.ngroups == b.ngroups && a.group0 == b.group0,
          "job %zu: final %d/%d nblocks %u/%u block0 %u/%u group_size %u/%u ngroups %u/%u group0 %u/%u", k, a.final_index, b.final_index, a.nblocks, b.nblocks, a.block0, b.block0,
          a.group_size, b.group_size, a.ngroups, b.ngroups, a.group0, b.group0);
  }
  // invariants: group sizes, the classes' group ranges, the block ranges
  uint64_t block_end = 0;
  uint32_t group_end[JC_COUNT] = {0};
  for (size_t k = 0; k < L.order.size(); k++) {
    const JobPlan& j = jobs[L.order[k]];
    CHECK(j.final_index == (int)k, "job at %zu has final_index %d", k, j.final_index);
    CHECK(k == 0 || jobs[L.order[k - 1]].cls <= j.cls, "class order at %zu", k);
    CHECK(j.group_size >= 1 && j.group_size <= 64 && (j.group_size & (j.group_size - 1)) == 0, "group_size %u", j.group_size);
    CHECK((uint64_t)j.ngroups * j.group_size >= j.nblocks && (uint64_t)(j.ngroups - 1) * j.group_size < j.nblocks, "ngroups %u of %u for %u blocks", j.ngroups, j.group_size, j.nblocks);
    CHECK(j.group0 == group_end[j.cls], "group0 %u, the class is at %u", j.group0, group_end[j.cls]);
    group_end[j.cls] += j.ngroups;
    CHECK(L.cls_first[j.cls] <= k && k < L.cls_first[j.cls + 1], "cls_first around %zu", k);
    if (L.fits) {
      CHECK(j.block0 % kJobTileBlocks == 0 && j.block0 == block_end, "block0 %u, the job before ends at %llu", j.block0, (unsigned long long)block_end);
      block_end += align_up(j.nblocks, kJobTileBlocks);
    }
  }
  for (int c = 0; c < JC_COUNT; c++) CHECK(group_end[c] == L.cls_groups[c], "class %d: %u groups, cls_groups %u", c, group_end[c], L.cls_groups[c]);
  if (L.fits) CHECK(block_end == L.total_blocks && L.total_blocks == (uint64_t)L.n_tiles * kJobTileBlocks, "total_blocks %llu", (unsigned long long)L.total_blocks);
  return L;
}

static LaneDeal check_lanes(const char* what, const std::vector<LaneRoot>& roots, uint64_t seq_all, int n_lanes, bool forced) {
  const RefLanes R = reference_lanes(roots, seq_all, n_lanes, forced);
  const LaneDeal D = deal_lanes(roots, seq_all, n_lanes, forced);
  CHECK(D.n_lanes == R.n_lanes, "n_lanes %d != %d", D.n_lanes, R.n_lanes);
  CHECK(D.call_z == R.call_z, "call_z %d != %d", D.call_z, R.call_z);
  CHECK(D.lane_of.size() == roots.size(), "lane_of has %zu entries for %zu roots", D.lane_of.size(), roots.size());
  for (size_t k = 0; k < roots.size() && k < D.lane_of.size(); k++) {
    int want = 0;
    for (size_t q = 0; q < R.w.size(); q++)
      if (R.w[q].second == roots[k].column_id) want = R.lane_of[q];
    CHECK(D.lane_of[k] == want, "root %u on lane %d, not %d", roots[k].column_id, D.lane_of[k], want);
    CHECK(D.lane_of[k] >= 0 && (D.lane_of[k] < D.n_lanes || D.n_lanes == 1), "root %u on lane %d of %d", roots[k].column_id, D.lane_of[k], D.n_lanes);
  }
  return D;
}

static void done(const char* what, int bad0, const std::string& note) {
  printf("%s: %s: %s\n", what, note.c_str(), g_bad == bad0 ? "same" : "DIFFERENT");
  g_cases++;
}

int main() {
  static_assert(kJobBlockBytes == RLE_BLK && kJobTileBlocks == RLE_TILE && kJobCodecByte == CODEC_BYTE, "the reference's constants");
  std::mt19937_64 rng(20240607);
  auto pick = [&](uint64_t n) { return (uint64_t)(rng() % n); };
  const int kDeep = JC_PRESENT1 + 255;
  const char* what;
  int bad0;

  // ---- layout: random calls ----
  what = "layout, random";
  bad0 = g_bad;
  for (int it = 0; it < 3000; it++) {
    static const int classes[] = {JC_PRESENT, JC_RLE2, JC_RLE1, JC_BYTE, JC_PRESENT1, JC_PRESENT1 + 1, JC_PRESENT1 + 7, kDeep};
    std::vector<JobPlan> jobs;
    const int nj = (int)pick(pick(4) ? 12 : 60);
    for (int k = 0; k < nj; k++) {
      const int cls = classes[pick(it % 3 ? 8 : 4)];
      const int codec = cls == JC_RLE2 ? CODEC_RLE2 : (cls == JC_RLE1 ? CODEC_RLE1 : CODEC_BYTE);
      uint64_t len = 0;
      switch (pick(6)) {
        case 0: len = pick(3) * 511; break;
        case 1: len = pick(1 << 12); break;
        case 2: len = (uint64_t)RLE_BLK * RLE_TILE * pick(4) + pick(3) - 1 + (pick(2) ? 1 : 0); break;
        case 3: len = pick(1ull << 26); break;
        case 4: len = (uint64_t)RLE_BLK * (510 + pick(5)) * (1 + pick(130)); break;
        default: len = pick(1ull << (10 + pick(24))); break;
      }
      if (len == ~0ull) len = 0;
      static const int widths[] = {1, 2, 4, 8, 16};
      const uint64_t expect = pick(5) ? pick(1 + len * (1 + pick(70))) : 0;
      jobs.push_back(job(cls, codec, len, expect, widths[pick(5)]));
    }
    check_layout(what, jobs);
  }
  done(what, bad0, "3000 calls");

  // ---- layout: by hand ----
  {
    what = "layout, no jobs";
    bad0 = g_bad;
    std::vector<JobPlan> jobs;
    const JobLayout L = check_layout(what, jobs);
    CHECK(L.fits && L.total_blocks == 0 && L.n_tiles == 0 && L.order.empty() && L.cls_first[JC_COUNT] == 0 && L.cls_tab0[JC_COUNT] == 0, "an empty call");
    done(what, bad0, "0 blocks");
  }
  {
    what = "layout, one empty stream";
    bad0 = g_bad;
    std::vector<JobPlan> jobs{job(JC_RLE2, CODEC_RLE2, 0, 0, 8)};
    const JobLayout L = check_layout(what, jobs);
    CHECK(jobs[0].nblocks == 1 && jobs[0].ngroups == 1 && jobs[0].group_size == 1 && L.total_blocks == RLE_TILE && L.n_tiles == 1 && L.call_blocks == 1, "nblocks %u", jobs[0].nblocks);
    done(what, bad0, "1 block");
  }
  {
    what = "layout, a class without a job between two used ones";
    bad0 = g_bad;
    std::vector<JobPlan> jobs{job(JC_RLE1, CODEC_RLE1, 5000, 100, 4), job(JC_PRESENT, CODEC_BYTE, 700, 100, 1), job(JC_RLE1, CODEC_RLE1, 100, 100, 4), job(JC_PRESENT, CODEC_BYTE, 1, 1, 1)};
    const JobLayout L = check_layout(what, jobs);
    CHECK(L.cls_first[JC_PRESENT] == 0 && L.cls_first[JC_RLE2] == 2 && L.cls_first[JC_RLE1] == 2 && L.cls_first[JC_BYTE] == 4 && L.cls_first[JC_COUNT] == 4, "cls_first");
    CHECK(L.cls_groups[JC_RLE2] == 0 && L.cls_tab0[JC_RLE2] == L.cls_tab0[JC_RLE1], "the empty class");
    CHECK((L.order == std::vector<int>{1, 3, 0, 2}), "stable order");
    done(what, bad0, "4 jobs");
  }
  {
    what = "layout, only the deepest PRESENT class";
    bad0 = g_bad;
    std::vector<JobPlan> jobs{job(kDeep, CODEC_BYTE, 4000, 32000, 1)};
    const JobLayout L = check_layout(what, jobs);
    CHECK(L.cls_first[kDeep] == 0 && L.cls_first[JC_COUNT] == 1 && L.cls_groups[kDeep] == jobs[0].ngroups && L.cls_tab0[kDeep] == 0 && L.cls_tab0[JC_COUNT] == jobs[0].ngroups, "class %d", kDeep);
    done(what, bad0, "1 job");
  }
  {
    what = "layout, byte RLE of 511, 512, 1023 and 1024 blocks";
    bad0 = g_bad;
    std::vector<JobPlan> jobs;
    for (uint64_t nb : {511, 512, 1023, 1024}) jobs.push_back(job(JC_BYTE, CODEC_BYTE, nb * RLE_BLK, 0, 1));
    check_layout(what, jobs);
    CHECK(jobs[0].nblocks == 511 && jobs[0].group_size == 1 && jobs[1].nblocks == 512 && jobs[1].group_size == 1, "511 / 512 blocks: groups of %u / %u", jobs[0].group_size, jobs[1].group_size);
    CHECK(jobs[2].group_size == 1 && jobs[3].group_size == 2 && jobs[3].ngroups == 512, "1023 / 1024 blocks: groups of %u / %u", jobs[2].group_size, jobs[3].group_size);
    done(what, bad0, "4 jobs");
  }
  {
    what = "layout, no expected values";
    bad0 = g_bad;
    // (64 before the caps: a stream of 64 x 64 blocks in a call of 64 x kGroupTarget keeps it)
    std::vector<JobPlan> jobs{job(JC_RLE2, CODEC_RLE2, 4096ull * RLE_BLK, 0, 8), job(JC_RLE1, CODEC_RLE1, (64 * kGroupTarget - 4096) * RLE_BLK, 1ull << 40, 8)};
    check_layout(what, jobs);
    CHECK(jobs[0].group_size == 64 && jobs[0].ngroups == 64, "group_size %u", jobs[0].group_size);
    CHECK(jobs[1].group_size == 1, "a stream that expands 2^40 values: group_size %u", jobs[1].group_size);
    done(what, bad0, "2 jobs");
  }
  {
    what = "layout, a call of 64 x kGroupTarget blocks and one block less";
    bad0 = g_bad;
    std::vector<JobPlan> at{job(JC_RLE2, CODEC_RLE2, 64 * kGroupTarget * RLE_BLK, 0, 8)}, below{job(JC_RLE2, CODEC_RLE2, (64 * kGroupTarget - 1) * RLE_BLK, 0, 8)};
    const JobLayout L = check_layout(what, at);
    check_layout(what, below);
    CHECK(L.call_blocks == 64 * kGroupTarget && at[0].group_size == 64 && below[0].group_size == 32, "groups of %u and %u", at[0].group_size, below[0].group_size);
    done(what, bad0, "2 calls");
  }
  {
    what = "layout, 2^32 blocks and one tile less";
    bad0 = g_bad;
    std::vector<JobPlan> over{job(JC_RLE2, CODEC_RLE2, (1ull << 31) * RLE_BLK, 0, 8), job(JC_BYTE, CODEC_BYTE, (1ull << 31) * RLE_BLK - 700, 0, 1)};
    std::vector<JobPlan> under{job(JC_RLE2, CODEC_RLE2, (1ull << 31) * RLE_BLK, 0, 8), job(JC_BYTE, CODEC_BYTE, ((1ull << 31) - RLE_TILE) * RLE_BLK, 0, 1)};
    const JobLayout A = check_layout(what, over), B = check_layout(what, under);
    CHECK(!A.fits && A.total_blocks == 1ull << 32, "2^32 blocks: fits %d", (int)A.fits);
    CHECK(B.fits && B.total_blocks == (1ull << 32) - RLE_TILE && B.n_tiles == (1u << 22) - 1, "2^32 - 1024 blocks: fits %d", (int)B.fits);
    done(what, bad0, "2 calls");
  }

  // ---- lanes: random calls ----
  what = "lanes, random";
  bad0 = g_bad;
  for (int it = 0; it < 4000; it++) {
    std::vector<LaneRoot> roots;
    const int nr = 1 + (int)pick(pick(3) ? 6 : 24);
    const uint32_t top = 1u << (6 + pick(14));
    for (int k = 0; k < nr; k++) {
      uint32_t id = 1 + (uint32_t)pick(200);
      for (bool again = true; again;) {
        again = false;
        for (auto& r : roots) again |= r.column_id == id;
        if (again) id = 1 + (uint32_t)pick(200);
      }
      const uint64_t bytes = pick(4) ? pick(1ull << (4 + pick(28))) : (uint64_t)(1 + pick(3)) << 20;  // (often equal)
      uint32_t mx = 0;
      switch (pick(5)) {
        case 0: mx = 0; break;
        case 1: mx = top; break;
        case 2: mx = top * 3 / 5 + (uint32_t)pick(3) - 1; break;
        case 3: mx = top / 2 + (uint32_t)pick(3) - 1; break;
        default: mx = (uint32_t)pick(top + 1); break;
      }
      roots.push_back(LaneRoot{id, bytes, std::min(mx, top)});
    }
    const uint64_t seq_all = pick(3) ? kZstdLanesMinSequences - 2 + pick(4) : pick(1ull << 28);
    check_lanes(what, roots, seq_all, 1 + (int)pick(4), pick(2) != 0);
  }
  done(what, bad0, "4000 calls");

  // ---- lanes: by hand ----
  const uint64_t few = 1000, many = kZstdLanesMinSequences;
  {
    what = "lanes, one root";
    bad0 = g_bad;
    const LaneDeal D = check_lanes(what, {{3, 1000, 0}}, few, 2, true);
    CHECK(D.n_lanes == 1 && D.lane_of[0] == 0 && D.call_z == 0, "n_lanes %d", D.n_lanes);
    done(what, bad0, "1 lane");
  }
  {
    what = "lanes, more lanes wanted than roots";
    bad0 = g_bad;
    const LaneDeal D = check_lanes(what, {{1, 500, 0}, {2, 400, 0}}, few, 4, true);
    CHECK(D.n_lanes == 2 && D.lane_of[0] == 0 && D.lane_of[1] == 1, "n_lanes %d", D.n_lanes);
    done(what, bad0, "2 lanes");
  }
  {
    what = "lanes, the first root a quarter of the call, and one byte less";
    bad0 = g_bad;
    // (closed: the lighter roots share lane 1 although lane 0 holds less than they do together)
    const LaneDeal Q = check_lanes(what, {{1, 100, 0}, {2, 99, 0}, {3, 99, 0}, {4, 99, 0}, {5, 3, 0}}, few, 2, true);
    CHECK(Q.lane_of[0] == 0 && Q.lane_of[1] == 1 && Q.lane_of[2] == 1 && Q.lane_of[3] == 1 && Q.lane_of[4] == 1, "a quarter: %d %d %d %d %d", Q.lane_of[0], Q.lane_of[1], Q.lane_of[2], Q.lane_of[3], Q.lane_of[4]);
    const LaneDeal R = check_lanes(what, {{1, 100, 0}, {2, 99, 0}, {3, 99, 0}, {4, 99, 0}, {5, 4, 0}}, few, 2, true);
    CHECK(R.lane_of[0] == 0 && R.lane_of[1] == 1 && R.lane_of[2] == 1 && R.lane_of[3] == 0 && R.lane_of[4] == 1, "a byte less: %d %d %d %d %d", R.lane_of[0], R.lane_of[1], R.lane_of[2], R.lane_of[3], R.lane_of[4]);
    done(what, bad0, "2 calls");
  }
  {
    what = "lanes, longest block of 4095 and of 4096 sequences";
    bad0 = g_bad;
    // (below 4096 the bytes alone decide; from 4096 on the root with the long block has lane 0 and the light ones the other)
    const LaneDeal A = check_lanes(what, {{1, 50, 4095}, {2, 40, 0}, {3, 30, 0}}, few, 2, true);
    CHECK(A.lane_of[0] == 0 && A.lane_of[1] == 1 && A.lane_of[2] == 1, "4095: %d %d %d", A.lane_of[0], A.lane_of[1], A.lane_of[2]);
    const LaneDeal B = check_lanes(what, {{1, 50, 0}, {2, 40, 4096}, {3, 30, 0}}, few, 2, true);
    CHECK(B.lane_of[0] == 1 && B.lane_of[1] == 0 && B.lane_of[2] == 1, "4096: %d %d %d", B.lane_of[0], B.lane_of[1], B.lane_of[2]);
    done(what, bad0, "2 calls");
  }
  {
    what = "lanes, two lanes with one sequence less than the table scale and at it";
    bad0 = g_bad;
    // (mx 5000 of 10000: heavy by the half rule, light by the three-fifths rule)
    const std::vector<LaneRoot> roots{{1, 10, 10000}, {2, 100, 5000}, {3, 60, 6000}, {4, 50, 100}};
    const LaneDeal A = check_lanes(what, roots, many - 1, 2, false);
    CHECK(A.call_z == 0 && A.lane_of[0] == 0 && A.lane_of[1] == 0 && A.lane_of[2] == 0 && A.lane_of[3] == 1, "below: %d %d %d %d", A.lane_of[0], A.lane_of[1], A.lane_of[2], A.lane_of[3]);
    const LaneDeal B = check_lanes(what, roots, many, 2, false);
    CHECK(B.call_z == 1 && B.lane_of[0] == 0 && B.lane_of[1] == 1 && B.lane_of[2] == 0 && B.lane_of[3] == 0, "at: %d %d %d %d", B.lane_of[0], B.lane_of[1], B.lane_of[2], B.lane_of[3]);
    done(what, bad0, "2 calls");
  }
  {
    what = "lanes, every root heavy";
    bad0 = g_bad;
    const std::vector<LaneRoot> roots{{1, 10, 9000}, {2, 20, 5000}, {3, 30, 4500}};
    const LaneDeal A = check_lanes(what, roots, few, 2, false);
    CHECK(A.n_lanes == 1, "automatic: %d lanes", A.n_lanes);
    const LaneDeal B = check_lanes(what, roots, few, 2, true);
    CHECK(B.n_lanes == 2 && B.lane_of[2] == 0 && B.lane_of[1] == 1 && B.lane_of[0] == 1, "forced: %d lanes", B.n_lanes);
    done(what, bad0, "2 calls");
  }
  {
    what = "lanes, four forced of which the last two stay empty";
    bad0 = g_bad;
    // (three heavy roots share lane 0; light roots go to the emptiest of lanes 1 .. 3, so the only one leaves lanes 2 and 3 empty)
    const LaneDeal D = check_lanes(what, {{1, 10, 9000}, {2, 20, 5000}, {3, 30, 10}, {4, 5, 8000}}, few, 4, true);
    CHECK(D.n_lanes == 2 && D.lane_of[0] == 0 && D.lane_of[1] == 0 && D.lane_of[2] == 1 && D.lane_of[3] == 0, "%d lanes: %d %d %d %d", D.n_lanes, D.lane_of[0], D.lane_of[1], D.lane_of[2], D.lane_of[3]);
    done(what, bad0, "4 lanes wanted");
  }
  {
    what = "lanes, equal weights";
    bad0 = g_bad;
    // (given in falling order of their ids: the lower id is dealt first all the same)
    const LaneDeal D = check_lanes(what, {{9, 64, 0}, {7, 64, 0}, {5, 64, 0}, {2, 64, 0}, {1, 64, 0}}, few, 3, true);
    CHECK(D.lane_of[4] == 0 && D.lane_of[3] == 1 && D.lane_of[2] == 2 && D.lane_of[1] == 0 && D.lane_of[0] == 1, "%d %d %d %d %d", D.lane_of[4], D.lane_of[3], D.lane_of[2], D.lane_of[1], D.lane_of[0]);
    done(what, bad0, "3 lanes");
  }
  printf("checked %d cases, %d mismatches\n", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
