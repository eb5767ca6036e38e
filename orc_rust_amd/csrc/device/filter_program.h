// filter_program.h -- the row filter's predicate as a post-order program: what the host compiles (orcgpu_filter_plan.inc) and
// filter_eval_kernel runs (filter_kernels.hip).  Plain C++: no HIP in here.
#pragma once
#include <stdint.h>

enum {
  FOP_CMP_INT = 0,     // Byte / Short / Int / Long / Date against an integer literal, as int64
  FOP_CMP_FLOAT = 1,   // Float / Double against a float literal, as double (IEEE: a NaN on either side makes all but NE false)
  FOP_CMP_BOOL = 2,    // Boolean, false < true
  FOP_CMP_STRING = 3,  // String / Varchar / Char / Binary by unsigned byte, the shorter being the smaller on a common prefix
  FOP_CMP_DEC128 = 4,  // Decimal against a Decimal128 literal the host has brought to the column's scale, as int128
  FOP_IS_NULL = 5,
  FOP_IS_NOT_NULL = 6,  // (every op up to here is a leaf that reads a column, every op up to FOP_CMP_DEC128 one that reads its values)
  FOP_UNKNOWN = 7,     // a comparison with the NULL literal
  FOP_TRUE = 8,        // AND of no children
  FOP_FALSE = 9,       // OR of no children
  FOP_AND = 10,        // pops two, pushes one
  FOP_OR = 11,
  FOP_NOT = 12,
  FOP_LIKE = 13,       // String / Varchar / Char against a compiled LIKE pattern: a leaf that reads its column's values, through the
                       // match bits filter_like_kernel leaves (cmp: LIKE_*, the pattern's shape; i: which of the program's mask planes)
  FOP_IN = 14,         // x IN (list): a leaf that reads its column's values, through the match bits filter_in_kernel leaves (cmp: IN_*
                       // flags; i: its mask plane, numbered with the LIKE planes; lit_off / lit_len: its hash set in the literal pool;
                       // lo: the FKIND_* its column must be decoded to)
  FOP_CMP_EXPR = 15,   // lhs OP rhs over two arithmetic expressions: a leaf that reads the values of every column either side names,
                       // through the TWO planes filter_expr_kernel leaves (cmp: ORCGPU_PRED_EQ .. _GE; i: its T plane, i + 1 its F plane,
                       // numbered with the LIKE / IN planes; lit_off / lit_len: the two op tables in the literal pool, see below; col: unused)
  FOP_IN_SET = 16      // x IN SET s: FOP_IN against the sealed table of a device-resident key set (key_set_kernels.hip), which lies
                       // in the layout below, kind IN_KEY_I64.  lit_off is the table's DEVICE ADDRESS, not an offset into the literal
                       // pool; lit_len its bytes; cmp: IN_HAS_NULL or 0; i: its mask plane, numbered with the LIKE / IN planes; lo:
                       // FKIND_INT.  filter_in_kernel probes it, filter_eval_kernel reads the plane as it reads FOP_IN's
};
// does this instruction read the values of column `col` (not only its validity)?
inline bool fop_reads_values(uint32_t op) { return op <= FOP_CMP_DEC128 || op == FOP_LIKE || op == FOP_IN || op == FOP_IN_SET; }
// FKIND_INT holds Timestamp columns decoded to int64 (seconds .. nanoseconds) as well: the host brings the literal to the unit
enum { FKIND_INT = 0, FKIND_FLOAT = 1, FKIND_BOOL = 2, FKIND_STRING = 3, FKIND_OTHER = 4 /* fixed width, null tests only */, FKIND_DEC128 = 5 };

// the FKIND_* the column of an instruction that reads values must be decoded to (lo: FilterInsn::lo, where FOP_IN keeps its own)
inline uint32_t fop_value_kind(uint32_t op, unsigned long long lo = 0) {
  return op == FOP_IN || op == FOP_IN_SET ? (uint32_t)lo : op == FOP_CMP_INT ? FKIND_INT : op == FOP_CMP_FLOAT ? FKIND_FLOAT : op == FOP_CMP_BOOL ? FKIND_BOOL : op == FOP_CMP_DEC128 ? FKIND_DEC128 : FKIND_STRING;
}

struct FilterInsn {
  uint32_t op;       // FOP_*
  uint32_t cmp;      // ORCGPU_PRED_EQ .. _GE; FOP_LIKE: LIKE_*; FOP_IN: IN_* flags
  uint32_t col;      // index into the FilterCol table
  uint32_t lit_len;  // strings: bytes of the literal (FOP_LIKE: of the compiled pattern)
  long long i;       // integer / Boolean literal; Decimal128: the literal's high word (signed); FOP_LIKE: its mask plane
  double f;          // float literal
  unsigned long long lit_off;  // strings: where the literal starts in the literal pool
  unsigned long long lo;       // Decimal128: the literal's low word (unsigned)
};

// ---- a compiled LIKE pattern, as it lies in the literal pool at lit_off (4-byte aligned, lit_len bytes) ----
//   uint32 shape (LIKE_*), flags (LIKE_ANCHOR_*), n_parts, n_elems (elements of all parts), then per part {uint32 first, n}: its
//   elements are [first, first + n) of the two byte arrays that follow: bytes[n_elems] (the literal byte) and ones[n_elems] (1: the
//   element is `_`, one code point).  The parts are what stands between the pattern's unescaped `%`, the empty ones left out.
// The limits (ORCGPU_LIKE_MAX_BYTES / _PARTS of include/orcgpu.h) let filter_like_kernel hold the whole of it in LDS.
enum {
  LIKE_ALL = 0,       // only `%`: every valid row matches, no value byte is read and no mask plane exists
  LIKE_PREFIX = 1,    // literal%
  LIKE_SUFFIX = 2,    // %literal
  LIKE_CONTAINS = 3,  // %literal%
  LIKE_GENERAL = 4    // anything else with a wildcard in it
};
enum { LIKE_ANCHOR_START = 1, LIKE_ANCHOR_END = 2 };
constexpr uint32_t kLikeMaxBytes = 1024, kLikeMaxParts = 64;
constexpr uint32_t kLikeHeaderWords = 4;
constexpr uint32_t kLikeBlobMax = (kLikeHeaderWords + 2 * kLikeMaxParts) * 4 + 2 * kLikeMaxBytes;

// ---- the hash set of an IN leaf, as it lies in the literal pool at lit_off (8-byte aligned, lit_len bytes, a multiple of 8) ----
//   header, 8 x uint32: key kind (IN_KEY_*), n_slots (a power of two, at least twice the keys), n_keys (distinct), the shortest and
//     the longest key in bytes (strings), flags (IN_*), the hash bits that are DROPPED (0: none -- every IN list; a key set built
//     under ORCGPU_KEY_SET_HASH_BITS: the complement of its hash mask), 0
//   occupancy, ceil(n_slots / 64) x uint64: bit s = slot s holds a key -- so every int64 is a legal key
//   slots -- IN_KEY_I64: n_slots x uint64, the key (integers and Timestamps as int64; floats: the bits of the double, with
//     -0.0 stored as 0.0 and no NaN); IN_KEY_DEC128: n_slots x {uint64 low, uint64 high}; IN_KEY_STRING: n_slots x {uint32 hash,
//     uint32 length, uint32 offset of the key's bytes from the table's start, uint32 0}, the bytes of all keys behind the slots
// Open addressing, linear probing: a key sits in the first free slot at or behind hash & (n_slots - 1), wrapping round.  A probe
// ends at the key, at a free slot, or after n_slots steps: a damaged table cannot spin.  The hash functions are the ones below,
// for the host that builds and the kernel that probes.
enum { IN_KEY_I64 = 0, IN_KEY_DEC128 = 1, IN_KEY_STRING = 2 };
enum {
  IN_HAS_NULL = 1,    // the list holds a NULL literal: a row that matches no key is UNKNOWN, not FALSE
  IN_NO_TABLE = 2,    // no key can equal a row, or a Boolean column: no hash set, no mask plane, nothing for filter_in_kernel
  IN_BOOL_FALSE = 4,  // Boolean column (with IN_NO_TABLE): false is in the list
  IN_BOOL_TRUE = 8    // ... true is
};
constexpr uint32_t kInHeaderBytes = 32;
constexpr uint32_t kInLdsBytes = 32768;  // a table of up to this many bytes is staged in LDS, a larger one is probed in global memory
#if defined(__HIPCC__)
#define FILTER_HD __host__ __device__
#else
#define FILTER_HD
#endif
FILTER_HD inline unsigned long long in_mix64(unsigned long long k) {  // (the finaliser of MurmurHash3)
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}
FILTER_HD inline uint32_t in_hash_i64(unsigned long long key) { return (uint32_t)in_mix64(key); }
FILTER_HD inline uint32_t in_hash_dec128(unsigned long long lo, unsigned long long hi) { return (uint32_t)in_mix64(lo ^ in_mix64(hi)); }
FILTER_HD inline uint32_t in_hash_bytes(const uint8_t* p, uint32_t n) {  // FNV-1a, then the 32-bit finaliser of MurmurHash3
  uint32_t h = 2166136261u;
  for (uint32_t k = 0; k < n; k++) h = (h ^ p[k]) * 16777619u;
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}
// a float column's key: the double's bits, -0.0 as 0.0 (the caller has left NaN out: it equals nothing)
FILTER_HD inline unsigned long long in_float_key(double v) {
  if (v == 0.0) v = 0.0;
  union {
    double d;
    unsigned long long u;
  } x;
  x.d = v;
  return x.u;
}

// Where a key's chain starts.  hash_mask: what of the hash counts -- all of it for an IN list, so that this is hash & mask; fewer
// bits (a key set built under ORCGPU_KEY_SET_HASH_BITS) start every chain in the table's LAST slots, so that long chains wrap round
// its end.
FILTER_HD inline uint32_t in_first_slot(uint32_t hash, uint32_t hash_mask, uint32_t mask) { return ((hash & hash_mask) + ~hash_mask) & mask; }

// The table as a probe sees it, and the int64 probe: for filter_in_kernel, and for the host that checks a table it has laid out
struct InTable {
  uint32_t kind, n_slots, min_len, max_len, bytes;  // n_slots = 0: no usable table, nothing matches
  uint32_t hash_mask;                               // what of a key's hash counts (all of it, but for a key set built under fewer bits)
  const unsigned long long* occ;
  const uint8_t* slots;
  const uint8_t* base;  // strings: key offsets count from here, and stay below `bytes`
};
// The header, checked against the table's bytes: a table whose parts do not fit is treated as empty.
FILTER_HD inline InTable in_table(const uint8_t* tab, uint32_t bytes) {
  InTable t = {};
  t.base = tab;
  if (bytes < kInHeaderBytes) return t;
  const uint32_t* h = reinterpret_cast<const uint32_t*>(tab);
  t.kind = h[0];
  t.n_slots = h[1];
  t.min_len = h[3];
  t.max_len = h[4];
  t.hash_mask = ~h[6];
  t.bytes = bytes;
  t.base = tab;
  const uint64_t occ_bytes = ((uint64_t)t.n_slots + 63) / 64 * 8, slot_bytes = t.kind == IN_KEY_I64 ? 8 : 16;
  if (t.kind > IN_KEY_STRING || t.n_slots < 2 || (t.n_slots & (t.n_slots - 1)) || kInHeaderBytes + occ_bytes + (uint64_t)t.n_slots * slot_bytes > bytes) t.n_slots = 0;
  t.occ = reinterpret_cast<const unsigned long long*>(tab + kInHeaderBytes);
  t.slots = tab + kInHeaderBytes + occ_bytes;
  return t;
}
// Linear probing from the hash's own slot: at most n_slots steps, ended by the key or by a free slot.
FILTER_HD inline bool in_probe_i64(const InTable& t, unsigned long long key) {
  const uint32_t mask = t.n_slots - 1;
  uint32_t s = in_first_slot(in_hash_i64(key), t.hash_mask, mask);
  for (uint32_t step = 0; step < t.n_slots; step++, s = (s + 1) & mask) {
    if (!((t.occ[s >> 6] >> (s & 63)) & 1)) return false;
    if (reinterpret_cast<const unsigned long long*>(t.slots)[s] == key) return true;
  }
  return false;
}

// ---- an expression leaf, as it lies in the literal pool at lit_off (8-byte aligned, lit_len bytes) ----
//   header, 4 x uint32: the class (FXC_*), the ops of the left side's program, the ops of the right side's, and d = the right
//     side's scale minus the left side's as an int32 (FXC_DEC: |d| <= 38; the side of the smaller scale is multiplied by 10^|d|
//     before the two are compared; else 0)
//   2 x uint64: 10^|d|, low and high word
//   the left side's program, then the right side's: AggExprOp records (agg_program.h, 24 bytes each), each program with its
//     AX_GATE ops in front
enum { FXC_INT = 0, FXC_DEC = 1, FXC_FLOAT = 2 };
constexpr uint32_t kExprHeaderBytes = 32, kExprOpBytes = 24;

constexpr uint32_t kFilterStack = 64;  // = ORCGPU_FILTER_MAX_DEPTH: a predicate of depth d needs at most d slots of the evaluation stack
