// device/bloom_build.hip -- the writer's Bloom filters (orcgpu_writer_set_bloom_filter): the bitset of every row group of one
// column of a stripe, bit for bit what Apache ORC's writer sets and what bloom_filter.rs / row_group_filter.rs probe.  The kernels
// read the stripe's device-resident form through the row index's tables (device/col_stats.hip: IxCol, the jobs' valid value
// counts, first values and first string bytes), so nulls never reach them.  A block is one row group, a lane one value:
//
//   hash   Byte .. Long: the value sign-extended to i64 through Thomas Wang's 64-bit hash (Java's signed shifts);
//          Float, Double: the value as a double, its bits as i64 with every NaN 0x7ff8000000000000 (Double.doubleToLongBits),
//          through the same hash; strings and binaries: ORC's Murmur3 hash64, seed 104729, over the value's bytes
//   bits   h1 the low, h2 the high signed 32-bit half; for i = 1 .. k: c = h1 + i * h2 (wrapping), c = ~c when negative, bit
//          c % (64 * words); bit b is bit b % 32 of dword b / 32, which is word b / 64 of the bitset written little-endian
//
//   bloom_lds_kernel      the bitset in LDS (32-bit LDS atomic OR), then written out with plain stores
//   bloom_global_kernel   a bitset above BLOOM_LDS_BYTES: 32-bit atomic OR on the zeroed output itself
// OR commutes: the bytes do not depend on how the device schedules the lanes.

#define BLOOM_LDS_BYTES (48u << 10)  // the largest bitset bloom_lds_kernel is launched with

__device__ __forceinline__ uint64_t bloom_hash_long_dev(int64_t value) {
  uint64_t key = (uint64_t)value;
  key = (~key) + (key << 21);
  key ^= (uint64_t)((int64_t)key >> 24);
  key = key + (key << 3) + (key << 8);
  key ^= (uint64_t)((int64_t)key >> 14);
  key = key + (key << 2) + (key << 4);
  key ^= (uint64_t)((int64_t)key >> 28);
  key = key + (key << 31);
  return key;
}

__device__ __forceinline__ uint64_t bloom_rotl(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }

// (the strings lie back to back at any alignment: bytes are loaded one by one)
__device__ uint64_t bloom_murmur3_dev(const uint8_t* p, uint64_t n) {
  const uint64_t C1 = 0x87c37b91114253d5ull, C2 = 0x4cf5ad432745937full;
  uint64_t h1 = 104729;
  const uint64_t nblocks = n / 8;
  for (uint64_t i = 0; i < nblocks; i++) {
    uint64_t k1 = 0;
    for (int b = 0; b < 8; b++) k1 |= (uint64_t)p[8 * i + b] << (8 * b);
    k1 *= C1;
    k1 = bloom_rotl(k1, 31);
    k1 *= C2;
    h1 ^= k1;
    h1 = bloom_rotl(h1, 27);
    h1 = h1 * 5 + 1390208809ull;
  }
  const uint32_t tn = (uint32_t)(n - 8 * nblocks);
  if (tn) {
    uint64_t k1 = 0;
    for (uint32_t b = 0; b < tn; b++) k1 |= (uint64_t)p[8 * nblocks + b] << (8 * b);
    k1 *= C1;
    k1 = bloom_rotl(k1, 31);
    k1 *= C2;
    h1 ^= k1;
  }
  h1 ^= n;
  h1 ^= h1 >> 33;
  h1 *= 0xff51afd7ed558ccdull;
  h1 ^= h1 >> 33;
  h1 *= 0xc4ceb9fe1a85ec53ull;
  h1 ^= h1 >> 33;
  return h1;
}

// the hash of valid value i of an integer or float column
__device__ __forceinline__ uint64_t bloom_hash_value(const IxCol& col, uint64_t i) {
  if (col.kind == WR_FLOAT) {
    const double x = col.elem == 4 ? (double)((const float*)col.vals)[i] : ((const double*)col.vals)[i];
    return bloom_hash_long_dev(x != x ? 0x7ff8000000000000ll : (int64_t)__double_as_longlong(x));
  }
  switch (col.elem) {
    case 1: return bloom_hash_long_dev(((const int8_t*)col.vals)[i]);
    case 2: return bloom_hash_long_dev(((const int16_t*)col.vals)[i]);
    case 4: return bloom_hash_long_dev(((const int32_t*)col.vals)[i]);
    default: return bloom_hash_long_dev(((const int64_t*)col.vals)[i]);
  }
}

// the k bits of one hash, OR-ed into `bits` (LDS or global) of m_bits bits
__device__ __forceinline__ void bloom_set(uint32_t* bits, uint64_t m_bits, uint32_t k, uint64_t hash64) {
  const uint32_t h1 = (uint32_t)hash64, h2 = (uint32_t)(hash64 >> 32);
  for (uint32_t i = 1; i <= k; i++) {
    int32_t c = (int32_t)(h1 + i * h2);
    if (c < 0) c = ~c;
    const uint64_t bit = (uint64_t)(uint32_t)c % m_bits;
    atomicOr(bits + (bit >> 5), 1u << (bit & 31));
  }
}

// row group g of column c (job c * G + g): every valid value's bits into `bits`.  scan: 256 u64 of LDS for the strings' offsets
__device__ __forceinline__ void bloom_group(const IxCol& col, uint64_t v0, uint64_t n, uint64_t b0, uint32_t k, uint64_t m_bits, uint32_t* bits, uint64_t* scan) {
  const uint32_t t = threadIdx.x;
  if (col.kind != WR_STRING) {
    for (uint64_t i = t; i < n; i += 256) bloom_set(bits, m_bits, k, bloom_hash_value(col, v0 + i));
    return;
  }
  uint64_t base = b0;  // the bytes before this chunk of 256 values
  for (uint64_t i0 = 0; i0 < n; i0 += 256) {
    const uint64_t i = i0 + t;
    const uint64_t len = i < n ? ix_len(col.vals, col.elem, v0 + i) : 0;
    scan[t] = len;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d *= 2) {
      const uint64_t a = t >= d ? scan[t - d] : 0;
      __syncthreads();
      scan[t] += a;
      __syncthreads();
    }
    const uint64_t at = base + scan[t] - len;
    const uint64_t chunk = scan[255];
    __syncthreads();
    base += chunk;
    if (i < n) bloom_set(bits, m_bits, k, bloom_murmur3_dev(col.data + at, len));
  }
}

// one column's filters: block g = row group g; out: G bitsets of `words` u64 each.  Dynamic LDS: words * 8 bytes
extern "C" __global__ void __launch_bounds__(256) bloom_lds_kernel(const IxCol* cols, uint32_t c, uint64_t G, const uint64_t* cnt, const uint64_t* vscan,
                                                                   const uint64_t* bscan, uint32_t k, uint32_t words, uint32_t* out) {
  extern __shared__ uint32_t bloom_bits[];
  __shared__ uint64_t scan[256];
  const uint64_t g = blockIdx.x, j = (uint64_t)c * G + g;
  const IxCol col = cols[c];
  const uint32_t nd = words * 2;
  for (uint32_t i = threadIdx.x; i < nd; i += 256) bloom_bits[i] = 0;
  __syncthreads();
  bloom_group(col, vscan[j] - vscan[(uint64_t)c * G], cnt[j], bscan[j] - bscan[(uint64_t)c * G], k, (uint64_t)words * 64, bloom_bits, scan);
  __syncthreads();
  uint32_t* o = out + g * nd;
  for (uint32_t i = threadIdx.x; i < nd; i += 256) o[i] = bloom_bits[i];
}

// ... the same into `out` itself, zeroed before the launch
extern "C" __global__ void __launch_bounds__(256) bloom_global_kernel(const IxCol* cols, uint32_t c, uint64_t G, const uint64_t* cnt, const uint64_t* vscan,
                                                                      const uint64_t* bscan, uint32_t k, uint64_t words, uint32_t* out) {
  __shared__ uint64_t scan[256];
  const uint64_t g = blockIdx.x, j = (uint64_t)c * G + g;
  const IxCol col = cols[c];
  bloom_group(col, vscan[j] - vscan[(uint64_t)c * G], cnt[j], bscan[j] - bscan[(uint64_t)c * G], k, words * 64, out + g * words * 2, scan);
}
