// device/writer_dict.hip -- the stripe writer's string dictionaries (orcgpu_writer.inc, orcgpu_writer_set_dictionary): a stripe's
// non-null strings of one column (their bytes back to back, their lengths) -> DICTIONARY_V2's three value streams.  The
// dictionary's entries stand in first-occurrence order: entry k is the k-th distinct byte string in row order, so nothing that
// is written depends on which lane reached the table first.
//
//   wd_len32_kernel   the rows' lengths as u32 (their exclusive scan: where each row's bytes start)
//   wd_insert_kernel  a lane per row into an open-addressing table: a slot holds a representative row (atomicCAS from EMPTY) and
//                     the smallest row seen with that string (atomicMin); equality is the bytes' and the length's, never the hash's
//   wd_flag_kernel    1 for the rows that are their slot's smallest row (their exclusive scan: the string's id; the total: d),
//                     and those rows' lengths (their exclusive scan: where the entry's bytes start; the total: the bytes)
//   wd_ids_kernel     every row's id (DATA) and, from the flagged rows, the entries' lengths (LENGTH), rows and starts
//   wd_gather_kernel  DICTIONARY_DATA: 16 bytes of the output per lane, stored as one
//
// No loop here waits for another lane: a probe sequence ends after as many steps as the table has slots and raises `bad`.

#define WD_EMPTY 0xffffffffu

// FNV-1a over dwords while 16 bytes are left (loaded as one), over bytes after them, then murmur3's finaliser
__device__ __forceinline__ uint32_t wd_hash(const uint8_t* p, uint32_t len) {
  uint32_t h = 0x811c9dc5u ^ len, k = 0;
  for (; k + 16 <= len; k += 16) {
    uint4 a;
    __builtin_memcpy(&a, p + k, 16);
    h = (h ^ a.x) * 0x01000193u;
    h = (h ^ a.y) * 0x01000193u;
    h = (h ^ a.z) * 0x01000193u;
    h = (h ^ a.w) * 0x01000193u;
    h ^= h >> 15;
  }
  for (; k < len; k++) h = (h ^ p[k]) * 0x01000193u;
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// two strings of one length, 16 bytes a step: a long value costs its lane len / 16 steps, not len
__device__ __forceinline__ bool wd_equal(const uint8_t* p, const uint8_t* q, uint32_t len) {
  uint32_t k = 0;
  for (; k + 16 <= len; k += 16) {
    uint4 a, b;
    __builtin_memcpy(&a, p + k, 16);
    __builtin_memcpy(&b, q + k, 16);
    if (a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w) return false;
  }
  for (; k < len; k++)
    if (p[k] != q[k]) return false;
  return true;
}

extern "C" __global__ void __launch_bounds__(256) wd_len32_kernel(const void* lens, int len_bytes, uint64_t n, uint32_t* len32) {
  const uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  len32[row] = len_bytes == 4 ? ((const uint32_t*)lens)[row] : (uint32_t)((const uint64_t*)lens)[row];
}

// rep / low: the table's two words per slot, all WD_EMPTY before the launch; slot_mask: slots - 1 (a power of two, >= 2 n);
// hash_mask: ORCGPU_DICT_HASH_BITS.  Only a row index goes through the table: the bytes were written by earlier launches.
extern "C" __global__ void __launch_bounds__(256) wd_insert_kernel(const uint8_t* data, const uint64_t* offs, const uint32_t* len32, uint32_t n, uint32_t* rep,
                                                                   uint32_t* low, uint32_t slot_mask, uint32_t hash_mask, uint32_t* slot_of, uint32_t* bad) {
  const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n) return;
  const uint32_t row = (uint32_t)gid;
  const uint32_t len = len32[row];
  const uint8_t* p = data + offs[row];
  uint32_t slot = (wd_hash(p, len) & hash_mask) & slot_mask;
  for (uint32_t probe = 0; probe <= slot_mask; probe++, slot = (slot + 1) & slot_mask) {
    uint32_t r = __hip_atomic_load(rep + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (r == WD_EMPTY) {
      const uint32_t old = atomicCAS(rep + slot, WD_EMPTY, row);
      r = old == WD_EMPTY ? row : old;
    }
    if (r == row || (r < n && len32[r] == len && wd_equal(data + offs[r], p, len))) {
      // (most rows find a smaller row there already: no atomic on the slot every equal row shares)
      if (__hip_atomic_load(low + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > row) atomicMin(low + slot, row);
      slot_of[row] = slot;
      return;
    }
  }
  *bad = 1;
  slot_of[row] = 0;
}

extern "C" __global__ void __launch_bounds__(256) wd_flag_kernel(const uint32_t* slot_of, const uint32_t* low, const uint32_t* len32, uint32_t n, uint32_t* flag,
                                                                 uint32_t* flag_len) {
  const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n) return;
  const uint32_t row = (uint32_t)gid;
  const bool first = low[slot_of[row]] == row;
  flag[row] = first;
  flag_len[row] = first ? len32[row] : 0;
}

// first_id / first_off: the scans of flag / flag_len.  ids, ent_len: in the width the LENGTH stream's encoder reads (id_bytes)
extern "C" __global__ void __launch_bounds__(256) wd_ids_kernel(const uint32_t* slot_of, const uint32_t* low, const uint32_t* flag, const uint64_t* first_id,
                                                                const uint64_t* first_off, const uint32_t* len32, uint32_t n, int id_bytes, void* ids, void* ent_len,
                                                                uint32_t* ent_row, uint64_t* ent_off, uint32_t* bad) {
  const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n) return;
  const uint32_t row = (uint32_t)gid;
  const uint32_t m = low[slot_of[row]];
  uint64_t id = 0;
  if (m < n) id = first_id[m];
  else *bad = 1;  // (a row whose probes ran out)
  if (id_bytes == 4) ((uint32_t*)ids)[row] = (uint32_t)id;
  else ((uint64_t*)ids)[row] = id;
  if (flag[row]) {
    const uint64_t k = first_id[row];
    if (id_bytes == 4) ((uint32_t*)ent_len)[k] = len32[row];
    else ((uint64_t*)ent_len)[k] = len32[row];
    ent_row[k] = row;
    ent_off[k] = first_off[row];
  }
}

// out: 16-byte aligned, with room for the last store's spare bytes.  A lane finds the entry its first byte lies in by bisection
// and walks on through the entries its 16 bytes cover.
extern "C" __global__ void __launch_bounds__(256) wd_gather_kernel(const uint8_t* data, const uint64_t* offs, const uint32_t* ent_row, const uint64_t* ent_off,
                                                                   const uint64_t* d_entries, const uint64_t* d_bytes, uint4* out) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t pos = t * 16, D = *d_bytes, d = *d_entries;
  if (pos >= D || !d) return;
  uint64_t lo = 0, hi = d;  // the last entry that starts at or before pos
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (ent_off[mid] <= pos) lo = mid;
    else hi = mid;
  }
  uint64_t k = lo;
  uint64_t end = k + 1 < d ? ent_off[k + 1] : D;
  const uint8_t* src = data + offs[ent_row[k]] - ent_off[k];
  union {
    uint8_t b[16];
    uint4 q;
  } u;
  u.q = make_uint4(0, 0, 0, 0);
#pragma unroll
  for (uint32_t j = 0; j < 16; j++) {
    const uint64_t at = pos + j;
    if (at < D) {
      while (at >= end && k + 1 < d) {
        k++;
        end = k + 1 < d ? ent_off[k + 1] : D;
        src = data + offs[ent_row[k]] - ent_off[k];
      }
      u.b[j] = src[at];
    }
  }
  out[t] = u.q;
}
