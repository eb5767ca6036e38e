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
  FOP_LIKE = 13        // String / Varchar / Char against a compiled LIKE pattern: a leaf that reads its column's values, through the
                       // match bits filter_like_kernel leaves (cmp: LIKE_*, the pattern's shape; i: which of the program's mask planes)
};
// does this instruction read the values of column `col` (not only its validity)?
inline bool fop_reads_values(uint32_t op) { return op <= FOP_CMP_DEC128 || op == FOP_LIKE; }
// FKIND_INT holds Timestamp columns decoded to int64 (seconds .. nanoseconds) as well: the host brings the literal to the unit
enum { FKIND_INT = 0, FKIND_FLOAT = 1, FKIND_BOOL = 2, FKIND_STRING = 3, FKIND_OTHER = 4 /* fixed width, null tests only */, FKIND_DEC128 = 5 };

struct FilterInsn {
  uint32_t op;       // FOP_*
  uint32_t cmp;      // ORCGPU_PRED_EQ .. _GE; FOP_LIKE: LIKE_*
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

constexpr uint32_t kFilterStack = 64;  // = ORCGPU_FILTER_MAX_DEPTH: a predicate of depth d needs at most d slots of the evaluation stack
