// lz_compress.hip -- ORC stream compression on the device: Snappy and LZ4 (the inverse of src/compression.rs:113-195 for those two
// codecs).  A stream is cut into chunks of at most block_size bytes; a chunk is a 3-byte little-endian header (len * 2 +
// is_original) followed by a raw Snappy block or a raw LZ4 block, or by the chunk's own bytes when compressing did not make it
// smaller.
//
// The streams of one call (a writer's stripe) go through one launch set, with their lengths read on the device:
//   1. lzc_plan_kernel: per stream, its chunk and segment counts and their exclusive prefix (the job table);
//   2. lzc_segment_kernel: a wavefront per SEGMENT (at most LZC_SEG bytes of a chunk) finds greedy matches: the 64 lanes hash 64
//      positions at once against an LDS table of the chunk's earlier positions (primed with up to LZC_SEG bytes before the
//      segment) and against the earlier lanes of the same step (shuffles); the first matching lane by ballot wins, the match is
//      extended 64 bytes per step.  Table conflicts are settled by atomicMax (the later position wins), so the result does not
//      depend on which lane's write lands last.  The segment writes
//      its BODY: everything after the literals in front of its first match -- the literals of that first run are the chunk's
//      business, because for LZ4 a segment's trailing literals belong to the next segment's first sequence (a sequence without
//      a match is legal only at the end of a block);
//   3. lzc_chunk_size_kernel: per chunk, its compressed size from the segments' records; an exclusive scan (enc_scan) places
//      every chunk in its stream;
//   4. lzc_compose_kernel: per chunk, header, Snappy preamble, each segment's first literal run and body, the trailing literals
//      -- or the original bytes -- and each stream's compressed length into d_lens.
// Matches stay inside their segment and inside 64 KiB (Snappy: copy-1 / copy-2 only; LZ4: 16-bit offsets), and keep LZ4's
// end-of-block rules for both codecs: the last 5 bytes of a chunk are literals, its last match starts at least 12 bytes before
// its end.
#pragma once

#define LZC_SEG 16384u       // bytes per segment (less when the block size is smaller)
#define LZC_HASH_BITS 12u    // LDS hash table: 4096 positions, 16 KiB
#define LZC_NONE 0xffffffffu

struct LzcStream {     // a stream of the call (host-filled)
  uint64_t in_off;     // its bytes at in + in_off
  uint64_t out_off;    // its chunks at out + out_off (room: the length + 3 bytes per chunk)
  uint64_t known;      // its length, or ~0: d_lens[i] holds it
};

struct LzcPlan {       // device-filled; entry n_streams holds the totals
  uint64_t len;
  uint64_t chunk0;     // index of the stream's first chunk among the call's
  uint64_t seg0;       // ... and of its first segment
};

struct LzcSeg {        // what a segment found, relative to its chunk's start
  uint32_t first_pos;  // start of its first match (LZC_NONE: no match)
  uint32_t first_len;
  uint32_t last_end;   // end of its last match
  uint32_t body_len;   // bytes of its body in the stage
};

#define LZC_JOBS_PER_ARG 48u
struct LzcJobArgs {
  uint32_t n, at;
  LzcStream s[LZC_JOBS_PER_ARG];
};

__device__ __forceinline__ uint32_t lzc_load4(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}
__device__ __forceinline__ uint32_t lzc_hash(uint32_t v) { return (v * 0x9E3779B1u) >> (32u - LZC_HASH_BITS); }

// the index of the last entry with key(i) <= x among n ascending ones (n >= 1, key(0) == 0)
template <typename F>
__device__ __forceinline__ uint32_t lzc_find(uint32_t n, uint64_t x, F key) {
  uint32_t lo = 0, hi = n;  // key(lo) <= x < key(hi)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (key(mid) <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- element sizes and writers --------------------------------------------------------------------------------------------------
// LZ4: token, literal length bytes, literals, offset, match length bytes (lz4_Block_format.md)
__device__ __forceinline__ uint32_t lz4_ext_len(uint32_t v) { return v >= 15 ? (v - 15) / 255 + 1 : 0; }
__device__ __forceinline__ uint32_t lz4_put_ext(uint8_t* o, uint32_t v) {  // the bytes after a nibble of 15
  if (v < 15) return 0;
  v -= 15;
  uint32_t k = 0;
  for (; v >= 255; v -= 255) o[k++] = 255;
  o[k++] = (uint8_t)v;
  return k;
}
// Snappy: literal element header (tag 00), copy-1 / copy-2 elements (format_description.txt)
__device__ __forceinline__ uint32_t snappy_lit_hdr_len(uint32_t L) {
  if (!L) return 0;
  const uint32_t n = L - 1;
  return n < 60 ? 1 : (n < 256 ? 2 : (n < 65536 ? 3 : (n < (1u << 24) ? 4 : 5)));
}
__device__ __forceinline__ uint32_t snappy_put_lit_hdr(uint8_t* o, uint32_t L) {
  if (!L) return 0;
  const uint32_t n = L - 1;
  if (n < 60) {
    o[0] = (uint8_t)(n << 2);
    return 1;
  }
  const uint32_t k = n < 256 ? 1 : (n < 65536 ? 2 : (n < (1u << 24) ? 3 : 4));
  o[0] = (uint8_t)((59 + k) << 2);
  for (uint32_t i = 0; i < k; i++) o[1 + i] = (uint8_t)(n >> (8 * i));
  return 1 + k;
}
__device__ __forceinline__ uint32_t snappy_copy_one(uint8_t* o, uint32_t off, uint32_t len, bool write) {  // len 4 .. 64
  if (len <= 11 && off < 2048) {
    if (write) {
      o[0] = (uint8_t)(1 | ((len - 4) << 2) | ((off >> 8) << 5));
      o[1] = (uint8_t)off;
    }
    return 2;
  }
  if (write) {
    o[0] = (uint8_t)(2 | ((len - 1) << 2));
    o[1] = (uint8_t)off;
    o[2] = (uint8_t)(off >> 8);
  }
  return 3;
}
__device__ __forceinline__ uint32_t snappy_copies(uint8_t* o, uint32_t off, uint32_t len, bool write) {  // len >= 4, off < 65536
  uint32_t k = 0;
  while (len >= 68) {
    k += snappy_copy_one(o + k, off, 64, write);
    len -= 64;
  }
  if (len > 64) {
    k += snappy_copy_one(o + k, off, 60, write);
    len -= 60;
  }
  return k + snappy_copy_one(o + k, off, len, write);
}
__device__ __forceinline__ uint32_t varint_len(uint64_t v) {
  uint32_t k = 1;
  while (v >= 0x80) {
    v >>= 7;
    k++;
  }
  return k;
}

// ---- 0. the host's stream table, through kernel arguments -----------------------------------------------------------------------
__global__ __launch_bounds__(64) void lzc_put_jobs_kernel(LzcJobArgs a, LzcStream* dst) {
  if (threadIdx.x < a.n) dst[a.at + threadIdx.x] = a.s[threadIdx.x];
}

// ---- 1. chunks and segments per stream ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void lzc_plan_kernel(const LzcStream* js, uint32_t n, uint64_t* d_lens, uint64_t B, uint32_t S, LzcPlan* plan) {
  __shared__ uint64_t sc[1024], ss[1024];
  __shared__ uint64_t base_c, base_s;
  const uint32_t t = threadIdx.x;
  if (t == 0) base_c = base_s = 0;
  __syncthreads();
  const uint64_t spc = (B + S - 1) / S;
  for (uint32_t i0 = 0; i0 < n; i0 += 1024) {
    const uint32_t i = i0 + t;
    uint64_t len = 0, nc = 0, nsg = 0;
    if (i < n) {
      len = js[i].known != ~0ull ? js[i].known : d_lens[i];
      nc = (len + B - 1) / B;
      if (nc) {
        const uint64_t last = len - (nc - 1) * B;
        nsg = (nc - 1) * spc + (last + S - 1) / S;
      }
      if (!len) d_lens[i] = 0;  // (no chunk will write it)
    }
    sc[t] = nc;
    ss[t] = nsg;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d *= 2) {  // inclusive scan
      const uint64_t a = t >= d ? sc[t - d] : 0, b = t >= d ? ss[t - d] : 0;
      __syncthreads();
      sc[t] += a;
      ss[t] += b;
      __syncthreads();
    }
    if (i < n) plan[i] = LzcPlan{len, base_c + sc[t] - nc, base_s + ss[t] - nsg};
    __syncthreads();
    if (t == 1023) {
      base_c += sc[t];
      base_s += ss[t];
    }
    __syncthreads();
  }
  if (t == 0) plan[n] = LzcPlan{0, base_c, base_s};
}

// ---- 2. matches per segment -----------------------------------------------------------------------------------------------------
// stage: LZC stride bytes per segment (lzc_stride); meta: a record per segment
__global__ __launch_bounds__(64) void lzc_segment_kernel(int codec, const uint8_t* in, const LzcStream* js, const LzcPlan* plan, uint32_t n_streams, uint64_t B,
                                                         uint32_t S, uint64_t stride, LzcSeg* meta, uint8_t* stage) {
  __shared__ uint32_t table[1u << LZC_HASH_BITS];  // position + 1 of the latest hashed position; 0: none
  const uint64_t gid = blockIdx.x;
  if (gid >= plan[n_streams].seg0) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t s = lzc_find(n_streams, gid, [&](uint32_t i) { return plan[i].seg0; });
  const uint64_t len = plan[s].len, spc = (B + S - 1) / S, local = gid - plan[s].seg0;
  const uint64_t k = local / spc, c0 = k * B;
  const uint32_t clen = (uint32_t)min(B, len - c0);
  const uint32_t b = (uint32_t)(local % spc) * S, e = min(b + S, clen);
  const uint8_t* ch = in + js[s].in_off + c0;
  uint8_t* out = stage + gid * stride;
  // a match ends at or before mend (in its segment, 5 bytes before the chunk's end); it may start at p when p + 4 <= mend and
  // p + 12 <= clen
  const uint32_t mend = min(e, clen >= 5 ? clen - 5 : 0u);
  const uint32_t pend = min(mend >= 4 ? mend - 3 : 0u, clen >= 12 ? clen - 11 : 0u);  // starts below pend
  for (uint32_t i = lane; i < (1u << LZC_HASH_BITS); i += 64) table[i] = 0;
  __syncthreads();
  const uint32_t prime0 = b > S ? b - S : 0;
  for (uint32_t q = prime0 + lane; q < b; q += 64)
    if (q + 4 <= clen) atomicMax(&table[lzc_hash(lzc_load4(ch + q))], q + 1);
  __syncthreads();
  uint32_t first_pos = LZC_NONE, first_len = 0, last_end = 0, nb = 0, prev_end = b;
  uint32_t pos = b;
  while (pos < pend) {
    const uint32_t p = pos + lane;
    const bool ok = p < pend;
    uint32_t h = 0, cand = 0, v = 0;
    bool m = false;
    if (ok) {
      v = lzc_load4(ch + p);
      h = lzc_hash(v);
      const uint32_t c = table[h];
      m = c != 0 && c - 1 < p && p - (c - 1) <= 65535u && lzc_load4(ch + c - 1) == v;
      cand = c - 1;
    }
    // the batch's own positions are not in the table yet: the nearest earlier lane with the same 4 bytes comes first
    bool near = false;
    for (uint32_t d = 1; d < 64; d++) {
      const uint32_t u = __shfl_up(v, d);
      if (!near && ok && lane >= d && u == v) {
        cand = p - d;
        m = near = true;
      }
      if (!__ballot(ok && !near && lane > d)) break;
    }
    const uint64_t mask = __ballot(m);
    const uint32_t f = mask ? (uint32_t)__builtin_ctzll(mask) : 64u;
    // (positions past the match's start stay out: the next step starts behind the match, and would find them ahead of it)
    if (ok && lane <= f) atomicMax(&table[h], p + 1);
    if (!mask) {
      pos += 64;
      continue;
    }
    const uint32_t mp = pos + f, mc = __shfl(cand, f);
    // extend, 64 bytes a step
    const uint32_t limit = mend - mp;
    uint32_t mlen = 4;
    while (mlen < limit) {
      const uint32_t i = mlen + lane;
      const uint64_t stop = __ballot(i >= limit || ch[mp + i] != ch[mc + i]);
      if (stop) {
        mlen += (uint32_t)__builtin_ctzll(stop);
        break;
      }
      mlen += 64;
    }
    mlen = min(mlen, limit);
    const uint32_t off = mp - mc;
    uint8_t hdr[24];  // (lane 0 writes the elements' bytes, all lanes copy literals)
    if (first_pos == LZC_NONE) {
      first_pos = mp;
      first_len = mlen;
      if (codec == 0) {  // Snappy: the first match's copies
        if (lane == 0) snappy_copies(out + nb, off, mlen, true);
        nb += snappy_copies(hdr, off, mlen, false);
      } else {  // LZ4: the first sequence's offset and match length bytes (its token is the chunk's)
        if (lane == 0) {
          out[nb] = (uint8_t)off;
          out[nb + 1] = (uint8_t)(off >> 8);
          lz4_put_ext(out + nb + 2, mlen - 4);
        }
        nb += 2 + lz4_ext_len(mlen - 4);
      }
    } else {
      const uint32_t L = mp - prev_end;
      uint32_t hl;
      if (codec == 0) {
        hl = snappy_lit_hdr_len(L);
        if (lane == 0) snappy_put_lit_hdr(out + nb, L);
      } else {
        hl = 1 + lz4_ext_len(L);
        if (lane == 0) {
          out[nb] = (uint8_t)((min(L, 15u) << 4) | min(mlen - 4, 15u));
          lz4_put_ext(out + nb + 1, L);
        }
      }
      for (uint32_t i = lane; i < L; i += 64) out[nb + hl + i] = ch[prev_end + i];
      nb += hl + L;
      if (codec == 0) {
        if (lane == 0) snappy_copies(out + nb, off, mlen, true);
        nb += snappy_copies(hdr, off, mlen, false);
      } else {
        if (lane == 0) {
          out[nb] = (uint8_t)off;
          out[nb + 1] = (uint8_t)(off >> 8);
          lz4_put_ext(out + nb + 2, mlen - 4);
        }
        nb += 2 + lz4_ext_len(mlen - 4);
      }
    }
    prev_end = last_end = mp + mlen;
    pos = prev_end;
  }
  if (lane == 0) meta[gid] = LzcSeg{first_pos, first_len, last_end, nb};
}

// ---- 3. / 4. per chunk -------------------------------------------------------------------------------------------------------------
struct LzcChunk {
  uint32_t s;           // stream
  uint64_t k, c0;       // chunk of the stream, its offset
  uint32_t clen, nseg;  // its bytes, its segments
  uint64_t seg0;        // its first segment (global)
};
__device__ __forceinline__ LzcChunk lzc_chunk(uint64_t cid, const LzcPlan* plan, uint32_t n_streams, uint64_t B, uint32_t S) {
  LzcChunk c;
  c.s = lzc_find(n_streams, cid, [&](uint32_t i) { return plan[i].chunk0; });
  c.k = cid - plan[c.s].chunk0;
  c.c0 = c.k * B;
  c.clen = (uint32_t)min(B, plan[c.s].len - c.c0);
  c.nseg = (c.clen + S - 1) / S;
  c.seg0 = plan[c.s].seg0 + c.k * ((B + S - 1) / S);
  return c;
}
// the literal run in front of a match, or at the end (then LZ4 writes a token without a match): header bytes
__device__ __forceinline__ uint32_t lzc_lit_hdr_len(int codec, uint32_t L) {
  return codec == 0 ? snappy_lit_hdr_len(L) : 1 + lz4_ext_len(L);
}
// the compressed bytes of a chunk (without its header)
__device__ uint64_t lzc_chunk_body_len(int codec, const LzcChunk& c, const LzcSeg* meta) {
  uint64_t T = codec == 0 ? varint_len(c.clen) : 0;
  uint32_t carry = 0;
  for (uint32_t g = 0; g < c.nseg; g++) {
    const LzcSeg m = meta[c.seg0 + g];
    if (m.first_pos == LZC_NONE) continue;
    const uint32_t L = m.first_pos - carry;
    T += lzc_lit_hdr_len(codec, L) + L + m.body_len;
    carry = m.last_end;
  }
  const uint32_t L = c.clen - carry;
  if (codec == 1 || L) T += lzc_lit_hdr_len(codec, L) + L;
  return T;
}

// chunk_size[cid] = 3 + its bytes; 0 for the ids past the last chunk (the grid covers a bound, and one more)
__global__ __launch_bounds__(64) void lzc_chunk_size_kernel(int codec, const LzcPlan* plan, uint32_t n_streams, uint64_t B, uint32_t S, const LzcSeg* meta,
                                                            uint32_t* chunk_size) {
  const uint64_t cid = blockIdx.x;
  if (threadIdx.x) return;
  if (cid >= plan[n_streams].chunk0) {
    chunk_size[cid] = 0;
    return;
  }
  const LzcChunk c = lzc_chunk(cid, plan, n_streams, B, S);
  const uint64_t T = lzc_chunk_body_len(codec, c, meta);
  chunk_size[cid] = 3 + (uint32_t)(T < c.clen ? T : c.clen);
}

// chunk_off: exclusive scan of chunk_size
__global__ __launch_bounds__(256) void lzc_compose_kernel(int codec, const uint8_t* in, const LzcStream* js, const LzcPlan* plan, uint32_t n_streams, uint64_t B,
                                                          uint32_t S, uint64_t stride, const LzcSeg* meta, const uint8_t* stage, const uint64_t* chunk_off,
                                                          uint8_t* out, uint64_t* d_lens) {
  const uint64_t cid = blockIdx.x;
  if (cid >= plan[n_streams].chunk0) return;
  const uint32_t t = threadIdx.x;
  const LzcChunk c = lzc_chunk(cid, plan, n_streams, B, S);
  const uint64_t first = plan[c.s].chunk0, nch = plan[c.s + 1].chunk0 - first;
  if (c.k == 0 && t == 0) d_lens[c.s] = chunk_off[first + nch] - chunk_off[first];
  const uint8_t* ch = in + js[c.s].in_off + c.c0;
  uint8_t* o = out + js[c.s].out_off + (chunk_off[cid] - chunk_off[first]);
  const uint64_t T = lzc_chunk_body_len(codec, c, meta);
  const bool original = T >= c.clen;
  const uint32_t hv = (original ? c.clen : (uint32_t)T) * 2 + (original ? 1 : 0);
  if (t == 0) {
    o[0] = (uint8_t)hv;
    o[1] = (uint8_t)(hv >> 8);
    o[2] = (uint8_t)(hv >> 16);
  }
  o += 3;
  if (original) {
    for (uint32_t i = t; i < c.clen; i += 256) o[i] = ch[i];
    return;
  }
  uint64_t at = 0;
  if (codec == 0) {  // preamble: the uncompressed length
    if (t == 0) {
      uint32_t v = c.clen;
      uint32_t k = 0;
      while (v >= 0x80) {
        o[k++] = (uint8_t)(v | 0x80);
        v >>= 7;
      }
      o[k] = (uint8_t)v;
    }
    at = varint_len(c.clen);
  }
  uint32_t carry = 0;
  for (uint32_t g = 0; g <= c.nseg; g++) {
    // a segment with a match: the literals [carry, first_pos), then its body; past the last: the trailing literals
    LzcSeg m{c.clen, 0, c.clen, 0};
    const bool tail = g == c.nseg;
    if (!tail) {
      m = meta[c.seg0 + g];
      if (m.first_pos == LZC_NONE) continue;
    }
    const uint32_t L = m.first_pos - carry;
    if (tail && codec == 0 && !L) break;
    const uint32_t hl = lzc_lit_hdr_len(codec, L);
    if (t == 0) {
      if (codec == 0) {
        snappy_put_lit_hdr(o + at, L);
      } else {
        o[at] = (uint8_t)((min(L, 15u) << 4) | (tail ? 0u : min(m.first_len - 4, 15u)));
        lz4_put_ext(o + at + 1, L);
      }
    }
    for (uint32_t i = t; i < L; i += 256) o[at + hl + i] = ch[carry + i];
    at += hl + L;
    if (tail) break;
    const uint8_t* body = stage + (c.seg0 + g) * stride;
    for (uint32_t i = t; i < m.body_len; i += 256) o[at + i] = body[i];
    at += m.body_len;
    carry = m.last_end;
  }
}
