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
  FOP_NOT = 12
};
// FKIND_INT holds Timestamp columns decoded to int64 (seconds .. nanoseconds) as well: the host brings the literal to the unit
enum { FKIND_INT = 0, FKIND_FLOAT = 1, FKIND_BOOL = 2, FKIND_STRING = 3, FKIND_OTHER = 4 /* fixed width, null tests only */, FKIND_DEC128 = 5 };

struct FilterInsn {
  uint32_t op;       // FOP_*
  uint32_t cmp;      // ORCGPU_PRED_EQ .. _GE
  uint32_t col;      // index into the FilterCol table
  uint32_t lit_len;  // strings: bytes of the literal
  long long i;       // integer / Boolean literal; Decimal128: the literal's high word (signed)
  double f;          // float literal
  unsigned long long lit_off;  // strings: where the literal starts in the literal pool
  unsigned long long lo;       // Decimal128: the literal's low word (unsigned)
};

constexpr uint32_t kFilterStack = 64;  // = ORCGPU_FILTER_MAX_DEPTH: a predicate of depth d needs at most d slots of the evaluation stack
