// export_kernels.hip -- device code of the device-resident exports (orcgpu_export_device.inc).
//
// unpack_bits_kernel: an Arrow bitmap (LSB first) -> one byte per bit, for consumers without a bitmap type (torch.bool).
// Memory bound: n / 8 bytes in, n bytes out, so the stores are what counts.  The output is cut into
//   head   the bytes in front of the first 16-byte boundary of `out` (0 .. 15),
//   body   whole 16-byte chunks, each aligned: ONE global_store_dwordx4 per lane, a wavefront's store 1 KiB contiguous,
//   tail   what is left behind the last whole chunk (0 .. 15).
// A body lane takes the 16 bits of its chunk: 2 input bytes when the head is a multiple of 8 bits (always, for an aligned `out`),
// else 3, shifted -- every byte it reads holds one of its own bits, so nothing beyond ceil(n / 8) input bytes is touched.  Head
// and tail bytes go one per lane, by the lanes behind the body's: nothing beyond n output bytes is written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// 8 bits -> 8 bytes of 0 / 1, bit k in byte k
__device__ __forceinline__ unsigned long long unpack8(uint32_t x) {
  // (x replicated into every byte; byte k keeps bit k alone; a non-zero byte + 0x7f carries into its own bit 7, never beyond)
  const unsigned long long spread = ((unsigned long long)(x & 0xffu) * 0x0101010101010101ull) & 0x8040201008040201ull;
  return ((spread + 0x7f7f7f7f7f7f7f7full) >> 7) & 0x0101010101010101ull;
}

constexpr uint32_t kUnpackBlock = 256;

__global__ __launch_bounds__(kUnpackBlock) void unpack_bits_kernel(const uint8_t* __restrict__ bits, uint64_t n, uint8_t* __restrict__ out, uint32_t head,
                                                                   uint64_t n_chunks) {
  const uint64_t t = (uint64_t)blockIdx.x * kUnpackBlock + threadIdx.x;
  if (t < n_chunks) {
    const uint64_t bit0 = (uint64_t)head + t * 16;  // bit0 + 15 < n
    const uint64_t b = bit0 >> 3;
    const uint32_t sh = (uint32_t)(bit0 & 7);
    uint32_t w = (uint32_t)bits[b] | ((uint32_t)bits[b + 1] << 8);
    if (sh) w |= (uint32_t)bits[b + 2] << 16;  // (bit0 + 15) / 8 = b + 2: the chunk's own last bit lives there
    w >>= sh;
    const unsigned long long lo = unpack8(w), hi = unpack8(w >> 8);
    uint4 v;
    v.x = (uint32_t)lo;
    v.y = (uint32_t)(lo >> 32);
    v.z = (uint32_t)hi;
    v.w = (uint32_t)(hi >> 32);
    *reinterpret_cast<uint4*>(out + bit0) = v;  // out + head is 16-byte aligned
    return;
  }
  // head and tail: one byte per lane
  const uint64_t e = t - n_chunks;
  const uint64_t body_end = (uint64_t)head + n_chunks * 16;
  uint64_t i;
  if (e < head) i = e;
  else i = body_end + (e - head);
  if (i >= n) return;
  out[i] = (uint8_t)((bits[i >> 3] >> (i & 7)) & 1u);
}
