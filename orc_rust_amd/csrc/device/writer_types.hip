// device/writer_types.hip -- the two ORC primitives the stripe writer (orcgpu_writer.inc) encodes as two value streams, brought
// from their Arrow form to what the existing encoders take.
//
//   wr_timestamp_kernel    Timestamp(unit): the valid rows' values -> the seconds since 2015 (DATA, signed RLE v2) and the
//                          nanosecond codes (SECONDARY, unsigned RLE v2), gathered; values the format cannot hold raise `bad`
//   wr_dec_lengths_kernel  Decimal128: the bytes of each valid row's zigzag varint (null rows 0); their scan places the bytes
//   wr_dec_pack_kernel     ... the varints one behind the other: a block stages its 256 rows' bytes in LDS and stores whole dwords
//   wr_fill16_kernel       the scale, once per valid value, as the i16 the SECONDARY stream's encoder reads

#define WR_TS_BASE 1420070400ll  // 2015-01-01 00:00:00 UTC, the seconds ORC's DATA stream counts from
#define WR_DEC_MAX_BYTES 19u     // a 128-bit zigzag value in 7-bit groups

// ORC's nanosecond code: trailing decimal zeros, two or more of them, are stripped and counted in the low three bits
__device__ __forceinline__ uint64_t wr_nano_code(uint32_t nanos) {
  if (!nanos) return 0;
  uint32_t m = nanos, z = 0;
  while (m % 10 == 0) m /= 10, z++;
  return z >= 2 ? ((uint64_t)m << 3) | (z - 1) : (uint64_t)nanos << 3;
}

// ups: units per second; npu: nanoseconds per unit.  A valid value v: S = floor(v / ups), N the rest in nanoseconds.  The reader
// takes a stored second below zero with N > 999999 for one second earlier (ORC-763), so such a second is stored one later; S = -1
// would be stored as 0, which no reader corrects, and a second whose distance to 2015 leaves i64 has no code either: `bad`.
extern "C" __global__ void __launch_bounds__(256) wr_timestamp_kernel(const uint8_t* validity, uint64_t n_rows, const uint64_t* word_off, const int64_t* values,
                                                                      int64_t ups, int64_t npu, int64_t* secs, uint64_t* nanos, uint32_t* bad) {
  const uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n_rows) return;
  if (!((validity[row >> 3] >> (row & 7)) & 1)) return;
  const uint64_t at = enc_valid_before(validity, n_rows, word_off, row);
  const int64_t v = values[row];
  int64_t S = v / ups, r = v - S * ups;
  if (r < 0) r += ups, S -= 1;
  const uint32_t N = (uint32_t)(r * npu);
  const bool late = S < 0 && N > 999999u;
  int64_t stored = S + (late ? 1 : 0);
  if ((late && S == -1) || stored < INT64_MIN + WR_TS_BASE) {
    *bad = 1;
    stored = WR_TS_BASE;
  }
  secs[at] = stored - WR_TS_BASE;
  nanos[at] = wr_nano_code(N);
}

// the stripe's form back to (second, nanosecond): what the statistics are taken over
__device__ __forceinline__ void wr_timestamp_of(int64_t stored, uint64_t code, int64_t& S, uint32_t& N) {
  const uint32_t z = (uint32_t)(code & 7);
  uint64_t m = code >> 3;
  if (z)
    for (uint32_t i = 0; i <= z; i++) m *= 10;
  N = (uint32_t)m;
  S = stored + WR_TS_BASE;
  if (S < 0 && N > 999999u) S -= 1;
}

__device__ __forceinline__ unsigned __int128 wr_dec_zigzag(uint64_t lo, uint64_t hi) {
  const __int128 v = (__int128)(((unsigned __int128)hi << 64) | lo);
  return ((unsigned __int128)v << 1) ^ (unsigned __int128)(v >> 127);
}
__device__ __forceinline__ uint32_t wr_dec_varint_len(unsigned __int128 z) {
  const uint64_t hi = (uint64_t)(z >> 64), lo = (uint64_t)z;
  const uint32_t bits = hi ? 128u - (uint32_t)__builtin_clzll(hi) : (lo ? 64u - (uint32_t)__builtin_clzll(lo) : 1u);
  return (bits + 6) / 7;
}

extern "C" __global__ void __launch_bounds__(256) wr_dec_lengths_kernel(const uint64_t* values, const uint8_t* validity, uint64_t n_rows, uint32_t* vlen) {
  const uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n_rows) return;
  const bool valid = (validity[row >> 3] >> (row & 7)) & 1;
  vlen[row] = valid ? wr_dec_varint_len(wr_dec_zigzag(values[2 * row], values[2 * row + 1])) : 0u;
}

// row_dst: exclusive scan of vlen.  A block's rows fill one span of `out`; it is staged in LDS at the span's own offset into its
// first dword, so that every dword the span covers whole goes out as one store and only its two ends go out as bytes.
// out: 4-byte aligned; nothing at or past `cap` is written.
extern "C" __global__ void __launch_bounds__(256) wr_dec_pack_kernel(const uint64_t* values, const uint8_t* validity, uint64_t n_rows, const uint64_t* row_dst,
                                                                     const uint32_t* vlen, uint8_t* out, uint64_t cap) {
  __shared__ uint32_t stage[(256 * WR_DEC_MAX_BYTES + 4 + 3) / 4];
  const uint64_t r0 = (uint64_t)blockIdx.x * 256, row = r0 + threadIdx.x;
  const uint64_t rl = min(r0 + 256, n_rows) - 1;
  const uint64_t base = row_dst[r0], total = row_dst[rl] + vlen[rl] - base;
  const uint32_t a = (uint32_t)(base & 3);
  uint8_t* sb = (uint8_t*)stage;
  if (row < n_rows && ((validity[row >> 3] >> (row & 7)) & 1)) {
    unsigned __int128 z = wr_dec_zigzag(values[2 * row], values[2 * row + 1]);
    const uint32_t len = vlen[row];
    const uint64_t o = a + (row_dst[row] - base);
    if (len <= WR_DEC_MAX_BYTES && o + len <= sizeof(stage))
      for (uint32_t k = 0; k < len; k++) {
        sb[o + k] = (uint8_t)((uint32_t)z & 0x7f) | (k + 1 < len ? 0x80 : 0);
        z >>= 7;
      }
  }
  __syncthreads();
  const uint64_t end = min((uint64_t)a + total, (uint64_t)sizeof(stage));  // the span in the stage: bytes [a, end)
  uint8_t* o0 = out + (base - a);                                           // the stage's byte 0
  for (uint64_t k = threadIdx.x; k * 4 < end; k += 256) {
    const uint64_t lo = k * 4, hi = lo + 4;
    if (base - a + hi > cap) {
      for (uint64_t i = max(lo, (uint64_t)a); i < min(hi, end) && base - a + i < cap; i++) o0[i] = sb[i];
    } else if (lo >= a && hi <= end) {
      ((uint32_t*)o0)[k] = stage[k];
    } else {
      for (uint64_t i = max(lo, (uint64_t)a); i < min(hi, end); i++) o0[i] = sb[i];
    }
  }
}

extern "C" __global__ void __launch_bounds__(256) wr_fill16_kernel(uint16_t* dst, uint64_t n, uint16_t v) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = v;
}
