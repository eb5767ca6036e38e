// lz_exec.h -- LZ77 execution stage of the block decompressors: ONE WORKGROUP PER ORC CHUNK.
//
// Replaces the copy half of zstd::Decoder (compression.rs:151-159): the entropy stage (zstd_entropy.h)
// has turned every Compressed_Block into a literal buffer and a table of {offset value, match length,
// literal length}; this kernel resolves the repeat offsets and executes the copies, block after block,
// in the order of the frame.
//
// Sequences are taken T at a time (one per thread):
//   * repeat offsets (RFC 8878 3.1.1.5) are a serial state machine over three registers; every sequence is
//     written as a transformation of that triple (each new register is a constant, or an old register minus
//     a count) and the transformations are composed with a block-wide prefix scan;
//   * a block-wide scan of the lengths gives every sequence its place; as many sequences as fit are
//     assembled in an LDS stage of 16 KiB: literals by all threads (4 bytes at a time, each dword finds its
//     sequence with a binary search over the literal prefix sums), the part of a match that lies before
//     the group straight from memory (already flushed), the part that lies inside the group by
//     multi-round resolution -- in every round the matches whose source bytes are all final copy, until
//     none is left (the first unresolved match can always go);
//   * the stage is flushed with 16-byte stores; ONE workgroup fence + barrier per group makes it readable
//     for the groups that follow (all waves of a workgroup share the CU's L1).
// A sequence that alone exceeds the stage is copied memory to memory by the whole workgroup.
//
// Snappy and LZ4 chunks come through the same code (MODE 1): lz_parse.h has turned them into 8-byte token records
// {length | copy flag, copy offset or position of the literal bytes in the payload}; a token is a sequence that has
// only literals or only a match, the literal bytes are read where they lie, there are no repeat offsets.
#pragma once

#ifndef LZX_STAGE
#define LZX_STAGE 8192u
#endif
#ifndef LZX_STAGE_WAVE
#define LZX_STAGE_WAVE 2048u  // stage of the one-wavefront workgroups (lz_exec_wave_kernel)
#endif
#define LZX_DONE 0xffffu
#define LZX_WATCHDOG 25000u  // polls (about 2 us each) a workgroup waits for the entropy kernel before it puts the chunk off
#define LZX_SEQ_PACKED 0xffffffffu  // lz_exec_block's `soa`: the block's sequences are 8-byte records (zseq_pack)
#define LZX_DEFERRED 0x57a7u  // ChunkDesc::diag of a chunk put off: the second launch (behind the entropy kernel) takes it

#include "decomp_tables.h"  // ZItem: one block of a frame, in output order

template <int T>
struct ExecLds {
  static constexpr uint32_t STAGE = T <= 64 ? LZX_STAGE_WAVE : LZX_STAGE;
  __attribute__((aligned(16))) uint8_t stage[STAGE + 64];
  __attribute__((aligned(16))) uint16_t ptr[STAGE + 64];  // per stage byte: the stage byte it copies (LZX_DONE: final)
  uint64_t wsum[T / 64];
  uint32_t wred[T / 64];
  uint32_t wrep[T / 64][6];
  // (workgroups of several wavefronts, groups of long literals: every 4 bytes of the group's literals find their sequence)
  uint32_t ilit[T > 64 ? T : 1];   // inclusive literal prefix of the group's sequences
  uint32_t sdst[T > 64 ? T : 1];   // stage index of each sequence's first literal byte
  uint32_t lsrc[T > 64 ? T : 1];   // where its literal bytes lie (offset from `lit`)
  uint32_t bc[16];    // broadcast slots
  uint32_t big[8][3]; // literals of more than a kilobyte: {length, stage index, source offset}
};

struct RepX {  // transformation of the repeat-offset triple: new register k = (tk == 3) ? vk : old[tk] - vk
  uint32_t t0, v0, t1, v1, t2, v2;
};
__device__ __forceinline__ RepX rep_identity() { return RepX{0, 0, 1, 0, 2, 0}; }
__device__ __forceinline__ void rep_pick(const RepX& f, uint32_t tag, uint32_t& t, uint32_t& v) {
  t = tag == 0 ? f.t0 : (tag == 1 ? f.t1 : f.t2);
  v = tag == 0 ? f.v0 : (tag == 1 ? f.v1 : f.v2);
}
__device__ __forceinline__ void rep_expr(const RepX& f, uint32_t gt, uint32_t gv, uint32_t& t, uint32_t& v) {
  if (gt == 3) {
    t = 3;
    v = gv;
  } else {
    uint32_t ft, fv;
    rep_pick(f, gt, ft, fv);
    t = ft;
    v = ft == 3 ? fv - gv : fv + gv;
  }
}
// g after f
__device__ __forceinline__ RepX rep_compose(const RepX& g, const RepX& f) {
  RepX r;
  rep_expr(f, g.t0, g.v0, r.t0, r.v0);
  rep_expr(f, g.t1, g.v1, r.t1, r.v1);
  rep_expr(f, g.t2, g.v2, r.t2, r.v2);
  return r;
}
// what one sequence does (RFC 8878 3.1.1.5): offset value > 3: a new offset; 1..3: a repeat offset, shifted by one when the
// sequence has no literals (3 then meaning "first repeat offset - 1")
__device__ __forceinline__ RepX rep_of_sequence(uint32_t ofv, uint32_t ll) {
  if (ofv > 3) return RepX{3, ofv - 3, 0, 0, 1, 0};
  const uint32_t idx = ofv - 1 + (ll == 0 ? 1u : 0u);
  if (idx == 0) return rep_identity();
  if (idx == 1) return RepX{1, 0, 0, 0, 2, 0};
  if (idx == 2) return RepX{2, 0, 0, 0, 1, 0};
  return RepX{0, 1, 0, 0, 1, 0};
}
template <int CTRL, int ROWS>
__device__ __forceinline__ RepX rep_dpp(const RepX& x) {  // the value `CTRL` lanes below (identity where there is none)
  RepX r;
  r.t0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x.t0, CTRL, ROWS, 0xf, false);
  r.v0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x.v0, CTRL, ROWS, 0xf, false);
  r.t1 = (uint32_t)__builtin_amdgcn_update_dpp(1, (int)x.t1, CTRL, ROWS, 0xf, false);
  r.v1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x.v1, CTRL, ROWS, 0xf, false);
  r.t2 = (uint32_t)__builtin_amdgcn_update_dpp(2, (int)x.t2, CTRL, ROWS, 0xf, false);
  r.v2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x.v2, CTRL, ROWS, 0xf, false);
  return r;
}
__device__ __forceinline__ RepX rep_wave_scan(RepX x) {  // inclusive: lane i = op_i after ... after op_0
  x = rep_compose(x, rep_dpp<0x111, 0xf>(x));
  x = rep_compose(x, rep_dpp<0x112, 0xf>(x));
  x = rep_compose(x, rep_dpp<0x114, 0xf>(x));
  x = rep_compose(x, rep_dpp<0x118, 0xf>(x));
  x = rep_compose(x, rep_dpp<0x142, 0xa>(x));
  x = rep_compose(x, rep_dpp<0x143, 0xc>(x));
  return x;
}

// ptr[i0 .. i0 + n) = v0, v0 + 1, ...: four marks a store
__device__ __forceinline__ void lds_iota16(uint16_t* p, uint32_t v0, uint32_t n) {
  uint64_t pat = (uint64_t)v0 * 0x0001000100010001ull + 0x0003000200010000ull;
  uint32_t k = 0;
  for (; k + 4 <= n; k += 4, pat += 0x0004000400040004ull) __builtin_memcpy(p + k, &pat, 8);
  if (n & 2u) {
    const uint32_t x = (uint32_t)pat;
    __builtin_memcpy(p + k, &x, 4);
    k += 2;
    pat >>= 32;
  }
  if (n & 1u) p[k] = (uint16_t)pat;
}

template <int T>
__device__ __forceinline__ uint64_t block_incl_scan_u64(ExecLds<T>& L, uint64_t v, uint32_t tid) {
  const uint32_t lane = tid & 63, wv = tid >> 6;
  uint64_t x = wave_incl_scan_u64(v, lane);
  if (T > 64) {
    if (lane == 63) L.wsum[wv] = x;
    __syncthreads();
    uint64_t add = 0;
    for (uint32_t k = 0; k < wv; k++) add += L.wsum[k];
    x += add;
    __syncthreads();
  }
  return x;
}
template <int T>
__device__ __forceinline__ uint32_t block_min_u32(ExecLds<T>& L, uint32_t v, uint32_t tid) {
  const uint32_t lane = tid & 63, wv = tid >> 6;
  for (int s = 32; s; s >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, s);
    v = o < v ? o : v;
  }
  if (T > 64) {
    if (lane == 0) L.wred[wv] = v;
    __syncthreads();
    uint32_t m = 0xffffffffu;
    for (uint32_t k = 0; k < T / 64; k++) m = L.wred[k] < m ? L.wred[k] : m;
    __syncthreads();
    v = m;
  }
  return v;
}
template <int T>
__device__ __forceinline__ uint32_t block_count(ExecLds<T>& L, bool p, uint32_t tid) {
  const uint32_t lane = tid & 63, wv = tid >> 6;
  uint32_t c = (uint32_t)__popcll(__ballot(p));
  if (T > 64) {
    if (lane == 0) L.wred[wv] = c;
    __syncthreads();
    c = 0;
    for (uint32_t k = 0; k < T / 64; k++) c += L.wred[k];
    __syncthreads();
  }
  return c;
}

// memory -> memory copy by the whole workgroup (ranges do not overlap)
template <int T>
__device__ __forceinline__ void wg_copy(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t tid) {
  uint32_t k = tid * 8;
  for (; k + 8 <= n; k += T * 8) st_u64(dst + k, ld_u64(src + k));
  for (uint32_t t = (n & ~7u) + tid; t < n; t += T) dst[t] = src[t];
}
template <int T>
__device__ __forceinline__ void wg_fill(uint8_t* dst, uint32_t v, uint32_t n, uint32_t tid) {
  const uint64_t pat = 0x0101010101010101ull * (v & 0xff);
  uint32_t k = tid * 8;
  for (; k + 8 <= n; k += T * 8) st_u64(dst + k, pat);
  for (uint32_t t = (n & ~7u) + tid; t < n; t += T) dst[t] = (uint8_t)v;
}
__device__ __forceinline__ void wg_release() {  // earlier stores of this workgroup become readable by all its waves
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __syncthreads();
}

// XXH64 (seed 0) of n bytes at p, by the workgroup: RFC 8878 3.1.1 Content_Checksum = its low 32 bits; libzstd behind the
// reference's zstd crate verifies it when the frame header flags one (compression.rs:151-159) and so does this path.  The
// algorithm is four serial 64-bit lanes over 32-byte stripes (lane i takes bytes [8 i, 8 i + 8) of every stripe) and a serial
// tail: lanes 0..3 of the first wavefront follow them, lane 0 finishes.  A 256 KiB frame is 8192 steps of ~40 cycles.
__device__ __forceinline__ uint64_t xxh_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
#define XXH_P1 0x9E3779B185EBCA87ull
#define XXH_P2 0xC2B2AE3D27D4EB4Full
#define XXH_P3 0x165667B19E3779F9ull
#define XXH_P4 0x85EBCA77C2B2AE63ull
#define XXH_P5 0x27D4EB2F165667C5ull
__device__ __forceinline__ uint64_t xxh_round(uint64_t acc, uint64_t in) { return xxh_rotl(acc + in * XXH_P2, 31) * XXH_P1; }
__device__ __forceinline__ uint64_t xxh_merge(uint64_t h, uint64_t v) { return (h ^ xxh_round(0, v)) * XXH_P1 + XXH_P4; }
template <int T>
__device__ __forceinline__ uint64_t wg_xxh64(ExecLds<T>& L, const uint8_t* p, uint32_t n, uint32_t tid) {
  if (tid < 64) {
    const uint32_t lane = tid;
    const uint32_t stripes = n / 32;
    uint64_t v = lane == 0 ? XXH_P1 + XXH_P2 : (lane == 1 ? XXH_P2 : (lane == 2 ? 0ull : 0ull - XXH_P1));
    if (lane < 4) {
      const uint8_t* q = p + 8 * lane;
      uint32_t s = 0;
      for (; s + 8 <= stripes; s += 8) {  // (eight loads in flight: the chain is the multiplications, not the memory)
        uint64_t w[8];
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = ld_u64(q + 32ull * (s + k));
#pragma unroll
        for (int k = 0; k < 8; k++) v = xxh_round(v, w[k]);
      }
      for (; s < stripes; s++) v = xxh_round(v, ld_u64(q + 32ull * s));
    }
    const uint64_t v1 = __shfl(v, 0), v2 = __shfl(v, 1), v3 = __shfl(v, 2), v4 = __shfl(v, 3);
    if (lane == 0) {
      uint64_t h;
      if (n >= 32) {
        h = xxh_rotl(v1, 1) + xxh_rotl(v2, 7) + xxh_rotl(v3, 12) + xxh_rotl(v4, 18);
        h = xxh_merge(h, v1);
        h = xxh_merge(h, v2);
        h = xxh_merge(h, v3);
        h = xxh_merge(h, v4);
      } else {
        h = XXH_P5;
      }
      h += (uint64_t)n;
      uint32_t o = stripes * 32;
      for (; o + 8 <= n; o += 8) h = xxh_rotl(h ^ xxh_round(0, ld_u64(p + o)), 27) * XXH_P1 + XXH_P4;
      if (o + 4 <= n) {
        h = xxh_rotl(h ^ (uint64_t)ld_u32(p + o) * XXH_P1, 23) * XXH_P2 + XXH_P3;
        o += 4;
      }
      for (; o < n; o++) h = xxh_rotl(h ^ p[o] * XXH_P5, 11) * XXH_P1;
      h ^= h >> 33;
      h *= XXH_P2;
      h ^= h >> 29;
      h *= XXH_P3;
      h ^= h >> 32;
      L.bc[14] = (uint32_t)h;
      L.bc[15] = (uint32_t)(h >> 32);
    }
  }
  __syncthreads();
  const uint64_t h = (uint64_t)L.bc[14] | (uint64_t)L.bc[15] << 32;
  __syncthreads();
  return h;
}

// Executes the nseq sequences of one compressed block.  `out`, `lp`, R[]: running output position, literal position and
// repeat offsets (uniform).  Returns 0 or a diagnostic code.
template <int T, int MODE>
__device__ __forceinline__ int lz_exec_block(ExecLds<T>& L, const uint32_t* seq, uint32_t nseq, const uint8_t* lit, uint32_t lit_kind, uint32_t lit_byte,
                                             uint32_t litn, uint8_t* dst, uint32_t cap, uint32_t frame_start, uint32_t& out, uint32_t* R,
                                             const uint32_t* progress, const uint32_t* seq_status, uint32_t tid PROF_PARM, uint32_t soa = 0) {
  const uint32_t lane = tid & 63, wv = tid >> 6;
  uint32_t lp = 0;
  uint32_t s = 0;
  uint32_t prof_groups = 0, prof_rounds = 0;
  // the records of the next group are fetched while the current one is assembled
  uint32_t pre_s = 0xffffffffu, pofv = 0, pml = 0, pll = 0, plsrc = 0;
  // MODE 0: the sequences may still be on their way (zstd_entropy_kernel runs beside this kernel): `avail` of them are known to
  // be in memory.  await(need) blocks until `need` are (or the entropy job has ended); nonzero = the job failed.
  uint32_t avail = MODE == 0 && progress ? 0u : nseq;
  auto await = [&](uint32_t need) -> int {
    if (avail >= need) return 0;
    if (tid == 0) {
      uint32_t a, stt;
      for (uint32_t spins = 0;; spins++) {
        stt = __hip_atomic_load(seq_status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a = __hip_atomic_load(progress, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a >= need || stt != ZSTD_PENDING) break;
        if (spins > L.bc[12]) {  // (bc[12]: the patience of this launch, LZX_WATCHDOG by default) the entropy kernel is not getting anywhere beside this one: make room, the chunk is taken again later
          stt = LZX_DEFERRED;
          L.bc[11] = 1;
          break;
        }
        __builtin_amdgcn_s_sleep(64);
      }
      L.bc[8] = stt == 0 ? nseq : a;
      L.bc[9] = stt;
    }
    __syncthreads();
    avail = L.bc[8];
    const uint32_t stt = L.bc[9];
    __syncthreads();
    return stt != ZSTD_PENDING && stt != 0 ? 1 : 0;
  };
  auto fetch = [&](uint32_t start) {
    pre_s = start;
    pofv = pml = pll = plsrc = 0;
    if (start < nseq && tid < nseq - start) {
      if (MODE == 0) {
        // (agent scope: written by another workgroup, possibly on another XCD, while this kernel runs)
        // Zstandard (soa = the block's sequence count rounded up to 4): three arrays -- offset values, match lengths, literal
        // lengths -- one behind the other; DEFLATE (soa = 0): 12-byte records
        if (soa == LZX_SEQ_PACKED) {
          // (one lane per block, zstd_lanes.h: 8-byte records, written by a kernel that has ended)
          zseq_unpack(reinterpret_cast<const uint2*>(seq)[start + tid], pofv, pml, pll);
        } else {
          const uint32_t* q = soa ? seq + (start + tid) : seq + 3ull * (start + tid);
          const uint32_t st1 = soa ? soa : 1u, st2 = soa ? 2u * soa : 2u;
          pofv = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          pml = __hip_atomic_load(q + st1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          pll = __hip_atomic_load(q + st2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      } else if (MODE == 1) {
        const uint2 r = reinterpret_cast<const uint2*>(seq)[start + tid];
        const bool cp = r.x & LZ_COPY;
        pml = cp ? r.x & ~LZ_COPY : 0;
        pll = cp ? 0 : r.x;
        pofv = r.y;  // copy: the offset; literals: where they lie
      } else {
        // LZ4: a sequence is a pair of records, literals then match (the block's last sequence has no match: zeros behind it)
        const uint4 r = reinterpret_cast<const uint4*>(seq)[start + tid];
        pll = r.x;
        plsrc = r.y;
        pml = r.z & ~LZ_COPY;
        pofv = r.w;
      }
    }
  };
  bool flushed_dirty = false;  // the previous group's flush has been issued but not yet waited for
  while (s < nseq) {
    PROF_MARK(0);
    prof_groups++;
    const uint32_t n = nseq - s < (uint32_t)T ? nseq - s : (uint32_t)T;
    if (pre_s != s) {
      if (MODE == 0 && await(s + n)) return 46;
      fetch(s);
    }
    const uint32_t ofv = pofv, ml = pml, ll = pll, lsrc_in = plsrc;
    PROF_MARK(1);
    // ---- repeat offsets ----
    RepX x = rep_identity();
    if (MODE == 0) {
    // Nearly every group (99.9 % of lineitem's 5.5 M) holds nothing but NEW offsets and plain repeats of the last one (offset value
    // 1 behind literals): the repeat offsets are then a stack that only new offsets push onto, and a lane finds the last three
    // pushes at or below itself in a ballot -- ~30 instructions where the general scan composes six rounds of transformations (~250).
    const bool special = tid < n && ofv <= 3 && !(ofv == 1 && ll != 0);
    if (T <= 64 && __ballot(special) == 0) {
      const unsigned long long newm = __ballot(tid < n && ofv > 3);
      const unsigned long long upto = newm & (lane == 63 ? ~0ull : (2ull << lane) - 1);  // pushes by lanes <= this one
      const int a = upto ? 63 - __builtin_clzll(upto) : -1;
      const unsigned long long u1 = a >= 0 ? upto & ~(1ull << a) : 0ull;
      const int b = u1 ? 63 - __builtin_clzll(u1) : -1;
      const unsigned long long u2 = b >= 0 ? u1 & ~(1ull << b) : 0ull;
      const int c = u2 ? 63 - __builtin_clzll(u2) : -1;
      const uint32_t va = (uint32_t)__shfl((int)ofv, a < 0 ? 0 : a) - 3u, vb = (uint32_t)__shfl((int)ofv, b < 0 ? 0 : b) - 3u, vc = (uint32_t)__shfl((int)ofv, c < 0 ? 0 : c) - 3u;
      // the stack after this lane: its pushes on top of the registers the group came with
      x.t0 = a >= 0 ? 3u : 0u;
      x.v0 = a >= 0 ? va : 0u;
      x.t1 = b >= 0 ? 3u : (a >= 0 ? 0u : 1u);
      x.v1 = b >= 0 ? vb : 0u;
      x.t2 = c >= 0 ? 3u : (b >= 0 ? 0u : (a >= 0 ? 1u : 2u));
      x.v2 = c >= 0 ? vc : 0u;
    } else {
    x = tid < n ? rep_of_sequence(ofv, ll) : rep_identity();
    x = rep_wave_scan(x);
    }
    }
    PROF_MARK(12);
    if (MODE == 0 && T > 64) {
      if (lane == 63) {
        L.wrep[wv][0] = x.t0; L.wrep[wv][1] = x.v0; L.wrep[wv][2] = x.t1; L.wrep[wv][3] = x.v1; L.wrep[wv][4] = x.t2; L.wrep[wv][5] = x.v2;
      }
      __syncthreads();
      RepX p = rep_identity();
      for (uint32_t k = 0; k < wv; k++) {
        const RepX g{L.wrep[k][0], L.wrep[k][1], L.wrep[k][2], L.wrep[k][3], L.wrep[k][4], L.wrep[k][5]};
        p = rep_compose(g, p);
      }
      x = rep_compose(x, p);
      __syncthreads();
    }
    const uint32_t r0 = R[0], r1 = R[1], r2 = R[2];
    auto eval = [&](uint32_t t, uint32_t v) -> uint32_t { return t == 3 ? v : (t == 0 ? r0 : (t == 1 ? r1 : r2)) - v; };
    const uint32_t off = MODE == 0 ? eval(x.t0, x.v0) : (ml ? ofv : 1u);
    const uint32_t mylsrc = MODE == 0 ? 0u : (MODE == 1 ? ofv : lsrc_in);  // where the literals lie
    PROF_MARK(2);
    // ---- positions ----
    const uint32_t tot = ll + ml;
    const uint64_t incl = block_incl_scan_u64<T>(L, ((uint64_t)ll << 32) | tot, tid);
    const uint32_t io = (uint32_t)incl, il = (uint32_t)(incl >> 32);
    const uint32_t a0 = (uint32_t)(reinterpret_cast<uintptr_t>(dst + out) & 15u);  // the stage keeps the 16-byte alignment of the output
    const bool fit = tid < n && (uint64_t)a0 + io <= ExecLds<T>::STAGE;
    const uint32_t nfit = block_count<T>(L, fit, tid);
    if (nfit == 0) {
      // the first sequence alone is larger than the stage: memory to memory, all threads
      if (tid == 0) {
        L.bc[0] = off; L.bc[1] = ml; L.bc[2] = ll; L.bc[3] = eval(x.t1, x.v1); L.bc[4] = eval(x.t2, x.v2); L.bc[5] = MODE == 0 ? lp : mylsrc;
      }
      __syncthreads();
      const uint32_t boff = L.bc[0], bml = L.bc[1], bll = L.bc[2], b1 = L.bc[3], b2 = L.bc[4], blsrc = L.bc[5];
      __syncthreads();
      if (boff == 0) return 41;
      if ((MODE == 0 && (uint64_t)lp + bll > litn) || (uint64_t)out + bll + bml > cap) return 42;
      if (bml && (uint64_t)boff > (uint64_t)(out - frame_start) + bll) return 43;
      if (lit_kind == 1) wg_fill<T>(dst + out, lit_byte, bll, tid);
      else wg_copy<T>(dst + out, lit + blsrc, bll, tid);
      wg_release();
      flushed_dirty = false;
      const uint8_t* srcp = dst + out + bll - boff;
      uint8_t* dp = dst + out + bll;
      if (boff >= bml) {
        wg_copy<T>(dp, srcp, bml, tid);
      } else {
        for (uint32_t k = tid; k < bml; k += T) dp[k] = srcp[k % boff];  // the first `boff` bytes repeat
      }
      wg_release();
      out += bll + bml;
      lp += bll;
      s += 1;
      R[0] = boff; R[1] = b1; R[2] = b2;
      continue;
    }
    if (tid == nfit - 1) {
      L.bc[0] = io; L.bc[1] = il; L.bc[2] = off; L.bc[3] = eval(x.t1, x.v1); L.bc[4] = eval(x.t2, x.v2);
    }
    const bool act = tid < nfit;
    const bool bad = act && (off == 0 || (MODE == 0 && (uint64_t)lp + il > litn) || (uint64_t)out + io > cap ||
                             ((MODE == 0 || ml) && (uint64_t)off > (uint64_t)(out - frame_start) + (io - ml)));
    if (T > 64 && act) {
      L.ilit[tid] = il;
      L.sdst[tid] = a0 + io - tot;
      if (MODE != 0) L.lsrc[tid] = mylsrc;
    }
    if (flushed_dirty) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the previous group's bytes must be in memory before any wave reads them
    flushed_dirty = false;
    const uint32_t nbad = block_count<T>(L, bad, tid);  // (its barriers also publish ilit / sdst / bc, and end the fence)
    if (nbad) return 44;
    const uint32_t g_out = L.bc[0], g_lit = L.bc[1];
    const uint32_t n0 = L.bc[2], n1 = L.bc[3], n2 = L.bc[4];
    PROF_MARK(3);
    // ---- everything this group needs from memory is requested at once: the next group's records, this group's literals
    // (first dword of every thread), the parts of its matches that lie before the group ----
    {
      // (only what is known to have arrived: the next turn waits for the rest)
      const uint32_t nxt = s + nfit, nn = nseq - nxt < (uint32_t)T ? nseq - nxt : (uint32_t)T;
      if (MODE != 0 || avail >= nxt + nn) fetch(nxt);
    }
    const uint32_t d = a0 + io - ml;           // stage index of the match
    const int sidx = (int)d - (int)off;        // ... of its source (negative: before the stage)
    uint32_t kf = 0;
    if (act && ml && sidx < (int)a0) {
      kf = (uint32_t)((int)a0 - sidx);
      kf = kf < ml ? kf : ml;
    }
    const uint8_t* gsrc = dst + out - (uint32_t)((int)a0 - sidx);  // only used when kf > 0
    uint64_t fv0 = 0, fv1 = 0;
    if (kf && kf <= 16) {
      fv0 = ld_u64(gsrc);
      if (kf > 8) fv1 = ld_u64(gsrc + 8);
    }
    // ---- literals: every sequence places its own (most have a few bytes or none: a load or two and byte stores); long ones are
    // taken by the wavefront one at a time, 8 bytes per lane and step.  (Before: every 4 bytes of the group's literals looked for
    // their sequence with a binary search over the prefix sums -- a third of the kernel's time at table scale.) ----
    // (... in a workgroup of several wavefronts a group whose literals are long on average -- 16 bytes and more per sequence: an
    // incompressible stream -- is shared out 4 bytes per thread and step instead: every thread finds its sequence by a binary search
    // over the prefix sums, all wavefronts carry the load)
    const bool coop = T > 64 && g_lit >= 16u * nfit;
    if (coop) {
      for (uint32_t u = tid; 4 * u < g_lit; u += T) {
        const uint32_t j0 = 4 * u;
        const uint32_t nb = g_lit - j0 < 4 ? g_lit - j0 : 4;
        uint32_t lo = 0, hi = nfit - 1;
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (L.ilit[mid] > j0) hi = mid;
          else lo = mid + 1;
        }
        uint32_t i = lo;
        uint32_t before = i ? L.ilit[i - 1] : 0;
        uint32_t lim = L.ilit[i];
        uint32_t word, wbase = j0;  // `word` holds the literal bytes from index wbase of the group's literals on
        if (MODE != 0) word = ld_u32(lit + L.lsrc[i] + (j0 - before));  // (up to 3 bytes behind the literal: ORC_PAD)
        else if (lit_kind == 1) word = 0x01010101u * (lit_byte & 0xff);
        else word = ld_u32(lit + lp + j0);
        for (uint32_t b = 0; b < nb; b++) {
          const uint32_t j = j0 + b;
          if (j >= lim) {
            do {
              before = lim;
              i++;
              lim = L.ilit[i];
            } while (j >= lim);
            if (MODE != 0) {
              word = ld_u32(lit + L.lsrc[i] + (j - before));
              wbase = j;
            }
          }
          L.stage[L.sdst[i] + (j - before)] = (uint8_t)(word >> (8 * (j - wbase)));
        }
      }
    } else {
      const uint32_t sd = a0 + io - tot;  // stage index of this sequence's first literal byte
      const uint32_t lsrc_off = MODE == 0 ? lp + il - ll : mylsrc;
      const bool rle = MODE == 0 && lit_kind == 1;
      const uint64_t pat = 0x0101010101010101ull * (lit_byte & 0xff);
      const uint32_t myll = act ? ll : 0u;
      if (myll && myll <= 16) {
        uint64_t v0 = pat, v1 = pat;
        if (!rle) {
          v0 = ld_u64(lit + lsrc_off);  // (up to 15 bytes behind the literal: slack of the literal buffers / ORC_PAD)
          if (myll > 8) v1 = ld_u64(lit + lsrc_off + 8);
        }
        lds_put8(L.stage + sd, v0, myll < 8 ? myll : 8u);
        if (myll > 8) lds_put8(L.stage + sd + 8, v1, myll - 8);
      }
      // (workgroups of several wavefronts: literals of a kilobyte and more are left to all of them, below)
      const uint32_t wave_max = T > 64 ? 1024u : 0xffffffffu;
      unsigned long long m = __ballot(myll > 16 && myll <= wave_max);
      while (m) {
        const uint32_t i = (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        const uint32_t en = (uint32_t)__builtin_amdgcn_readlane((int)myll, (int)i);
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)sd, (int)i);
        const uint32_t es = (uint32_t)__builtin_amdgcn_readlane((int)lsrc_off, (int)i);
        for (uint32_t k = lane * 8; k < en; k += 512) {
          const uint64_t v = rle ? pat : ld_u64(lit + es + k);
          if (k + 8 <= en) __builtin_memcpy(L.stage + e0 + k, &v, 8);
          else
            for (uint32_t t = 0; k + t < en; t++) L.stage[e0 + k + t] = (uint8_t)(v >> (8 * t));
        }
      }
      if (T > 64) {
        // the longest ones by the whole workgroup, one after the other (their owners file them; few fit a stage)
        if (tid == 0) L.bc[13] = 0;
        __syncthreads();
        if (myll > wave_max) {
          const uint32_t slot = atomicAdd(&L.bc[13], 1u);
          if (slot < 8) {
            L.big[slot][0] = myll;
            L.big[slot][1] = sd;
            L.big[slot][2] = lsrc_off;
          }
        }
        __syncthreads();
        const uint32_t nbig = L.bc[13];  // (a stage of 8 KiB holds at most 7 literals of more than 1 KiB)
        for (uint32_t b = 0; b < nbig && b < 8; b++) {
          const uint32_t en = L.big[b][0], e0 = L.big[b][1], es = L.big[b][2];
          for (uint32_t k = tid * 8; k < en; k += T * 8) {
            const uint64_t v = rle ? pat : ld_u64(lit + es + k);
            if (k + 8 <= en) __builtin_memcpy(L.stage + e0 + k, &v, 8);
            else
              for (uint32_t t = 0; k + t < en; t++) L.stage[e0 + k + t] = (uint8_t)(v >> (8 * t));
          }
        }
      }
    }
    PROF_MARK(4);
    // ---- matches: the part before the group comes from memory ----
    if (kf && kf <= 16) {
      lds_put8(L.stage + d, fv0, kf < 8 ? kf : 8u);
      if (kf > 8) lds_put8(L.stage + d + 8, fv1, kf - 8);
    }
    {
      // long ones: the wave takes them one at a time, 8 bytes per lane and step
      unsigned long long m = __ballot(kf > 16);
      while (m) {
        const uint32_t i = (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        const uint32_t ekf = (uint32_t)__builtin_amdgcn_readlane((int)kf, (int)i);
        const uint32_t ed = (uint32_t)__builtin_amdgcn_readlane((int)d, (int)i);
        const uint32_t esrc = (uint32_t)__builtin_amdgcn_readlane((int)(out - (uint32_t)((int)a0 - sidx)), (int)i);
        const uint8_t* gp = dst + esrc;
        for (uint32_t k = lane * 8; k < ekf; k += 512) {
          const uint64_t v = ld_u64(gp + k);
          if (k + 8 <= ekf) __builtin_memcpy(L.stage + ed + k, &v, 8);
          else
            for (uint32_t t = 0; k + t < ekf; t++) L.stage[ed + k + t] = (uint8_t)(v >> (8 * t));
        }
      }
    }
    PROF_MARK(5);
    // ---- matches: the part inside the group, BYTE parallel.  Every byte of such a part points at the stage byte it repeats
    // (ptr[]); final bytes are marked LZX_DONE.  Each thread owns a span of the group's bytes and, round after round, either
    // copies a byte whose source has become final or makes it point at its source's source (pointer jumping: a chain of
    // k copies resolves in log2 k rounds, whether it runs through many matches or through one match that overlaps itself).
    // LDS executes a wavefront's operations in order, so a thread that sees ptr[q] == LZX_DONE also sees stage[q]. ----
    const uint32_t g_end = a0 + g_out;
    const uint32_t g_end8 = (g_end + 7u) & ~7u;
    for (uint32_t u = tid * 8; u < g_end8; u += T * 8) {
      const uint64_t dn[2] = {~0ull, ~0ull};
      __builtin_memcpy(&L.ptr[u], dn, 16);
    }
    __syncthreads();
    PROF_MARK(10);
    {
      // short parts by their thread; long ones by the wavefront, one at a time (a thread alone on a long match holds up the group)
      const uint32_t nin = act && kf < ml ? ml - kf : 0u;
      if (nin && nin <= 32) lds_iota16(&L.ptr[d + kf], d + kf - off, nin);
      unsigned long long m = __ballot(nin > 32);
      while (m) {
        const uint32_t i = (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        const uint32_t en = (uint32_t)__builtin_amdgcn_readlane((int)nin, (int)i);
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)(d + kf), (int)i);
        const uint32_t eo = (uint32_t)__builtin_amdgcn_readlane((int)off, (int)i);
        for (uint32_t k = lane; k < en; k += 64) L.ptr[e0 + k] = (uint16_t)(e0 + k - eo);
      }
    }
    // every thread owns a span of the stage (a multiple of 8 bytes, 8-byte aligned) and takes it 8 bytes at a time: the 8
    // marks with one read, then the 8 marks they point at, then the 8 bytes there -- independent reads, not a chain per byte
    const uint32_t span = (((g_end8 + T - 1) / T) + 7u) & ~7u;
    const uint32_t p0 = tid * span, p1 = p0 + span < g_end8 ? p0 + span : g_end8;
    __syncthreads();
    PROF_MARK(11);
    for (;;) {
      prof_rounds++;
      uint32_t open = 0;
      // three sweeps per barrier: a stale mark only points further from the byte's origin than necessary, never wrong
#pragma unroll 1
      for (int sweep = 0; sweep < 3; sweep++) {
      open = 0;
      for (uint32_t pp = p0; pp < p1; pp += 8) {
        uint32_t qw[4];
        __builtin_memcpy(qw, &L.ptr[pp], 16);
        if ((qw[0] & qw[1] & qw[2] & qw[3]) == 0xffffffffu) continue;
        uint32_t q[8], pq[8], sb[8];
#pragma unroll
        for (int i = 0; i < 8; i++) q[i] = (qw[i >> 1] >> (16 * (i & 1))) & 0xffffu;
#pragma unroll
        for (int i = 0; i < 8; i++) pq[i] = *(volatile uint16_t*)&L.ptr[q[i] == LZX_DONE ? 0u : q[i]];
        asm volatile("" ::: "memory");  // the marks first, then the bytes: a final mark vouches for its byte
#pragma unroll
        for (int i = 0; i < 8; i++) sb[i] = *(volatile uint8_t*)&L.stage[q[i] == LZX_DONE ? 0u : q[i]];
        uint64_t bytes;
        __builtin_memcpy(&bytes, &L.stage[pp], 8);
        uint32_t nw[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 8; i++) {
          uint32_t np = q[i];
          if (q[i] != LZX_DONE) {
            if (pq[i] == LZX_DONE) {
              bytes = (bytes & ~(0xffull << (8 * i))) | ((uint64_t)sb[i] << (8 * i));
              np = LZX_DONE;
            } else {
              np = pq[i];
              open++;
            }
          }
          nw[i >> 1] |= np << (16 * (i & 1));
        }
        __builtin_memcpy(&L.stage[pp], &bytes, 8);
        asm volatile("" ::: "memory");  // the bytes first, then their marks
        __builtin_memcpy(&L.ptr[pp], nw, 16);
      }
      if (!open) break;
      }
      if (!block_count<T>(L, open != 0, tid)) break;
    }
    PROF_MARK(6);
    // ---- flush: stage[a0, a0 + g_out) -> dst[out, out + g_out) ----
    {
      uint8_t* gbase = dst + out - a0;  // 16-byte aligned like the stage
      const uint32_t end = a0 + g_out;
      for (uint32_t u = tid; 16 * u < end; u += T) {
        const uint32_t lo = 16 * u, hi = lo + 16;
        if (lo >= a0 && hi <= end) {
          uint64_t v[2];
          __builtin_memcpy(v, L.stage + lo, 16);
          __builtin_memcpy(gbase + lo, v, 16);
        } else {
          // (the first and the last unit of a group: their bytes as aligned pieces of 1, 2, 4, 8 bytes -- at most seven stores where a
          // loop over the bytes made up to fifteen trips: 3 % of the kernel.  Measured beside it and not kept: the wavefront's long
          // literals two or four at a time with their loads in flight together (registers: 12 / 29 spilled), groups without a match
          // part inside the group skipping the marks and rounds (nearly every group has one))
          uint32_t b0 = lo < a0 ? a0 : lo;
          const uint32_t b1 = hi > end ? end : hi;
          if (b0 < b1 && (b0 & 1u)) { gbase[b0] = L.stage[b0]; b0 += 1; }
          if (b0 + 2 <= b1 && (b0 & 2u)) { uint16_t x; __builtin_memcpy(&x, L.stage + b0, 2); __builtin_memcpy(gbase + b0, &x, 2); b0 += 2; }
          if (b0 + 4 <= b1 && (b0 & 4u)) { uint32_t x; __builtin_memcpy(&x, L.stage + b0, 4); __builtin_memcpy(gbase + b0, &x, 4); b0 += 4; }
          if (b0 + 8 <= b1) { uint64_t x; __builtin_memcpy(&x, L.stage + b0, 8); __builtin_memcpy(gbase + b0, &x, 8); b0 += 8; }
          if (b0 + 4 <= b1) { uint32_t x; __builtin_memcpy(&x, L.stage + b0, 4); __builtin_memcpy(gbase + b0, &x, 4); b0 += 4; }
          if (b0 + 2 <= b1) { uint16_t x; __builtin_memcpy(&x, L.stage + b0, 2); __builtin_memcpy(gbase + b0, &x, 2); b0 += 2; }
          if (b0 < b1) gbase[b0] = L.stage[b0];
        }
      }
    }
    out += g_out;
    lp += g_lit;
    s += nfit;
    R[0] = n0; R[1] = n1; R[2] = n2;
    PROF_MARK(7);
    flushed_dirty = true;
    __syncthreads();  // the stage is free again (its bytes are on their way to memory: fenced before the next group reads them)
    PROF_MARK(8);
  }
  if (flushed_dirty) wg_release();
  PROF_COUNT(0, prof_groups);
  PROF_COUNT(1, prof_rounds);
  if (MODE != 0) return 0;
  // literals behind the last sequence
  const uint32_t rest = litn - lp;
  if ((uint64_t)out + rest > cap) return 45;
  if (rest) {
    if (lit_kind == 1) wg_fill<T>(dst + out, lit_byte, rest, tid);
    else wg_copy<T>(dst + out, lit + lp, rest, tid);
    out += rest;
    wg_release();
  }
  return 0;
}

// TOKENS: the instantiation for Snappy / LZ4 chunks (more threads: their sequences are short), else Zstandard chunks and copies
template <int T, bool TOKENS>
__device__ __forceinline__ void lz_exec_chunk(ExecLds<T>& L, uint32_t c, ChunkDesc* chunks, const ZItem* items, const ZBlock* zblocks, const uint32_t* zstatus,
                                              const uint32_t* zprogress, uint32_t n_zblocks, int copy_too, int retry) {
  const uint32_t tid = threadIdx.x;
  // retry: 0 = the launch beside the entropy kernel (may put chunks off), 1 = the launch behind it (only what the first one put
  // off), 2 = the only launch, behind the entropy kernel.  1 and 2 are FINAL: a chunk that still cannot be taken is an error there.
  if (retry == 1 && chunks[c].diag != LZX_DEFERRED) return;
  if (tid == 0) L.bc[11] = 0;
  __syncthreads();
  PROF_BEGIN();
  ChunkDesc d = chunks[c];
  const bool is_tok = d.kind == 2 || d.kind == 4;
  if ((d.kind == 0 && !copy_too) || is_tok != TOKENS) return;
  if (d.kind == 1 && (d.diag == LZX_DEFERRED || !d.scratch)) return;  // DEFLATE chunk left to the one-wavefront decoder
  if (d.kind == 3) return;                                             // LZO: decompress_lzo_kernel
  const uint8_t* src = as_global(d.src);
  uint8_t* dst = (uint8_t*)as_global((void*)d.dst);
  int st = 0;
  uint32_t out = 0;
  if (d.kind == 0) {
    if (d.src_len > d.dst_cap) st = 1;
    else {
      wg_copy<T>(dst, src, d.src_len, tid);
      out = d.src_len;
    }
  } else if (d.status) {
    st = 2;  // rejected by the host's parse of the frame / block headers, or by lz_parse_kernel
  } else if (TOKENS) {
    // Snappy / LZ4: the chunk's tokens (lz_parse.h); Snappy states the length, LZ4 may fill the slot
    uint32_t R[3] = {1, 4, 8};
    const uint32_t* recs = (const uint32_t*)as_global((void*)d.scratch);
    if (d.kind == 2) {
      st = lz_exec_block<T, 1>(L, recs, d.n_items, src, 0, 0, 0, dst, d.pad, 0, out, R, nullptr, nullptr, tid PROF_ARG);
      if (!st && out != d.pad) st = 35;
    } else {
      st = lz_exec_block<T, 2>(L, recs, (d.n_items + 1) / 2, src, 0, 0, 0, dst, d.dst_cap, 0, out, R, nullptr, nullptr, tid PROF_ARG);
    }
  } else if (d.kind == 1) {
    // DEFLATE: literal bytes + {distance + 3, match length, literal length} records from inflate_parse_kernel
    uint32_t R[3] = {1, 4, 8};
    const uint8_t* lit = (const uint8_t*)as_global((void*)d.scratch);
    const uint32_t* recs = reinterpret_cast<const uint32_t*>(lit + ((d.dst_cap + 16 + 15) & ~15u));
    st = lz_exec_block<T, 0>(L, recs, d.n_items, lit, 2, 0, d.pad, dst, d.dst_cap, 0, out, R, nullptr, nullptr, tid PROF_ARG);
    if (st) {
      // anything wrong with a DEFLATE chunk is the serial decoder's to report
      if (tid == 0) L.bc[11] = 1;
      __syncthreads();
    }
  } else if (d.kind != 5) {
    st = 3;  // unknown compression kind
  } else if (!TOKENS) {
    uint32_t R[3] = {1, 4, 8};
    uint32_t frame_start = 0;
    const uint32_t cap = d.dst_cap;
    for (uint32_t k = 0; k < d.n_items && !st; k++) {
      const ZItem it = items[d.first_item + k];
      if (it.flags & 1) {
        frame_start = out;
        R[0] = 1; R[1] = 4; R[2] = 8;
      }
      if (it.kind == 0) {
        if ((uint64_t)out + it.size > cap) st = 31;
        else {
          wg_copy<T>(dst + out, src + it.src_off, it.size, tid);
          out += it.size;
          wg_release();
        }
      } else if (it.kind == 1) {
        if ((uint64_t)out + it.size > cap) st = 32;
        else {
          wg_fill<T>(dst + out, it.src_off, it.size, tid);
          out += it.size;
          wg_release();
        }
      } else {
        const ZBlock* zb = zblocks + it.zblock;
        const uint32_t* zst = (const uint32_t*)as_global((void*)zstatus);
        // the literals job of the block must have ended (its bytes are read with ordinary loads: acquire); the sequences are taken
        // as they arrive
        auto job_end = [&](uint32_t job) -> uint32_t {
          if (tid == 0) {
            uint32_t v;
            uint32_t spins = 0;
            while ((v = __hip_atomic_load(zst + job, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == ZSTD_PENDING) {
              if (++spins > L.bc[12]) {
                v = LZX_DEFERRED;
                L.bc[11] = 1;
                break;
              }
              __builtin_amdgcn_s_sleep(64);
            }
            L.bc[10] = v;
          }
          __syncthreads();
          const uint32_t v = L.bc[10];
          __syncthreads();
          return v;
        };
        if (job_end(n_zblocks + it.zblock)) st = 33;
        else {
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          const uint8_t* lit = it.lit_kind == 2 ? as_global((const uint8_t*)zb->lit_out) : src + it.lit_off;
          const uint32_t block_start = out;
          // matches count from the start of the frame: positions are relative to the chunk's slot, the frame's first byte is frame_start
          st = lz_exec_block<T, 0>(L, (const uint32_t*)as_global((void*)zb->seq_out), it.nseq, lit, it.lit_kind, it.lit_off, it.litn, dst, cap, frame_start, out,
                                R, (const uint32_t*)as_global((void*)(zprogress + it.zblock)), zst + it.zblock, tid PROF_ARG, it.seq_packed ? LZX_SEQ_PACKED : (it.nseq + 3u) & ~3u);
          if (!st && job_end(it.zblock)) st = 33;  // (a block without sequences, or a job that failed behind the last one)
          if (!st && out - block_start > it.size) st = 36;  // more than Block_Maximum_Size regenerated (inside the slot: `cap` held)
        }
      }
      if (!st && (it.flags & 2) && (uint64_t)(out - frame_start) != it.fcs) st = 34;
      if (!st && (it.flags & 4)) {
        // the frame's content checksum (its bytes are in memory: every block ends with a workgroup release)
        const uint64_t h = wg_xxh64<T>(L, dst + frame_start, out - frame_start, tid);
        if ((uint32_t)h != ld_u32(src + it.ck_off)) st = 35;
      }
    }
  }
  PROF_MARK(9);
  PROF_END_AT(80);
  __syncthreads();
  if (tid == 0) {
    const bool put_off = L.bc[11] != 0 && retry == 0;  // (its status stays clear: the second launch decides)
    // a final launch that still meets a pending status word (an entropy job that never wrote it) reports the chunk: never a
    // silent "ok" with nothing decoded
    chunks[c].out_len = st ? 0 : out;
    chunks[c].status = st && !put_off ? ORC_E_CODEC : 0;
    chunks[c].diag = put_off ? LZX_DEFERRED : (uint32_t)st;
    // the entropy kernel is not getting anywhere beside this workgroup: do not wait again for the rest of its queue (each wait is
    // LZX_WATCHDOG polls long), put everything not ready at once off to the launch behind
    if (put_off) L.bc[12] = 0;
  }
}
#ifndef LZX_THREADS
#define LZX_THREADS 256
#endif
#ifndef LZT_THREADS
#define LZT_THREADS 1024
#endif
// Zstandard chunks and copies.  The kernel runs beside zstd_entropy_kernel and waits for its output, so it must never keep that
// kernel from being dispatched: the grid is small enough to be resident at once (the host sizes it by the CU count) and its
// workgroups take chunks from a queue -- `order`: the chunks with the most sequences first -- until it is empty.  Should the entropy
// kernel still not get anywhere (a workgroup waits LZX_WATCHDOG polls at most), the chunk is put off and a second launch of this kernel
// behind the entropy kernel (`retry`) takes it: slower, never wrong, never stuck.
#ifndef LZX_MIN_WAVES
#define LZX_MIN_WAVES 4
#endif
extern "C" __global__ void __launch_bounds__(LZX_THREADS, LZX_MIN_WAVES) lz_exec_kernel(ChunkDesc* chunks, uint32_t n_chunks, const ZItem* items, const ZBlock* zblocks, const uint32_t* zstatus, const uint32_t* zprogress,
                                                                         uint32_t n_zblocks, int copy_too, const uint32_t* order, uint32_t* next_chunk, int retry, uint32_t patience) {
  __shared__ ExecLds<LZX_THREADS> L;
  __shared__ uint32_t take;
  if (threadIdx.x == 0) L.bc[12] = patience;
  if (!next_chunk) {
    // one chunk per workgroup (behind the entropy stage, nothing to wait for): the dispatcher deals the workgroups out, kernels of
    // other streams get their turn as workgroups end -- a persistent grid holds every CU until its queue is empty
    if (blockIdx.x < n_chunks) lz_exec_chunk<LZX_THREADS, false>(L, order[blockIdx.x], chunks, items, zblocks, zstatus, zprogress, n_zblocks, copy_too, retry);
    return;
  }
  for (;;) {
    if (threadIdx.x == 0) {
      // beside the entropy kernel this grid is kept small (it must not keep that kernel from being placed); once every entropy
      // job has ended there is nothing left to wait for: the chunks not taken yet go to the launch behind, which is larger
      const bool entropy_over = retry == 0 && n_zblocks &&
                                __hip_atomic_load(next_chunk + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 2u * n_zblocks;
      take = entropy_over ? 0xffffffffu : atomicAdd(next_chunk, 1u);
    }
    __syncthreads();
    const uint32_t k = take;
    __syncthreads();
    if (k >= n_chunks) break;
    lz_exec_chunk<LZX_THREADS, false>(L, order[k], chunks, items, zblocks, zstatus, zprogress, n_zblocks, copy_too, retry);
    __syncthreads();
  }
}
// Table scale (zstd_lanes.h ran the entropy stage: nothing to wait for): ONE WAVEFRONT per chunk, groups of 64 sequences in a 2 KiB
// stage.  The four-wavefront workgroups above win when a call is as long as its longest chunk; when there are thousands of chunks
// per CU-slot what counts is chunks in flight and time per sequence: 16 chunks per CU instead of 4, scans and counts without LDS
// round trips or barriers between wavefronts (SF 12.5: the execution phase 22 -> 14 ms).  One chunk per workgroup, no queue.
#ifndef LZX_WAVE_MIN_WAVES
#define LZX_WAVE_MIN_WAVES 4
#endif
extern "C" __global__ void __launch_bounds__(64, LZX_WAVE_MIN_WAVES) lz_exec_wave_kernel(ChunkDesc* chunks, uint32_t n_chunks, const ZItem* items, const ZBlock* zblocks, const uint32_t* zstatus,
                                                                                   const uint32_t* zprogress, uint32_t n_zblocks, int copy_too, const uint32_t* order) {
  __shared__ ExecLds<64> L;
  if (threadIdx.x == 0) L.bc[12] = LZX_WATCHDOG;
  if (blockIdx.x < n_chunks) lz_exec_chunk<64, false>(L, order[blockIdx.x], chunks, items, zblocks, zstatus, zprogress, n_zblocks, copy_too, 2);
}
extern "C" __global__ void __launch_bounds__(LZT_THREADS) lz_exec_tokens_kernel(ChunkDesc* chunks, uint32_t n_chunks) {
  __shared__ ExecLds<LZT_THREADS> L;
  if (blockIdx.x < n_chunks) lz_exec_chunk<LZT_THREADS, true>(L, blockIdx.x, chunks, nullptr, nullptr, nullptr, nullptr, 0, 0, 0);
}
// ... with four wavefronts per chunk: for calls whose chunks fill the device several times over (lineitem SF 4, 4.7 k chunks: Snappy
// 17.6 -> 15.7 ms, LZ4 18.2 -> 16.4 ms -- the barriers of sixteen wavefronts cost more than their lanes bring); a call of few chunks
// (C3: 240) lasts as long as one chunk takes and is better off with sixteen (2.9 against 3.4 ms)
extern "C" __global__ void __launch_bounds__(256) lz_exec_tokens4_kernel(ChunkDesc* chunks, uint32_t n_chunks) {
  __shared__ ExecLds<256> L;
  if (blockIdx.x < n_chunks) lz_exec_chunk<256, true>(L, blockIdx.x, chunks, nullptr, nullptr, nullptr, nullptr, 0, 0, 0);
}
