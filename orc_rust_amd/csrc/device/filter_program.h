// filter_program.h -- the row filter's predicate as a post-order program: what the host compiles (orcgpu_filter_plan.inc) and
// filter_eval_kernel runs (filter_kernels.hip).  Plain C++: no HIP in here.
#pragma once
#include <stdint.h>

enum {
  FOP_CMP_INT = 0,     // Byte / Short / Int / Long / Date against an integer literal, as int64
  FOP_CMP_FLOAT = 1,   // Float / Double against a float literal, as double (IEEE: a NaN on either side makes all but NE false)
  FOP_CMP_BOOL = 2,    // Boolean, false < true
  FOP_CMP_STRING = 3,  // String / Varchar / Char / Binary by unsigned byte, the shorter being the smaller on a common prefix
  FOP_IS_NULL = 4,
  FOP_IS_NOT_NULL = 5,
  FOP_UNKNOWN = 6,     // a comparison with the NULL literal
  FOP_TRUE = 7,        // AND of no children
  FOP_FALSE = 8,       // OR of no children
  FOP_AND = 9,         // pops two, pushes one
  FOP_OR = 10,
  FOP_NOT = 11
};
enum { FKIND_INT = 0, FKIND_FLOAT = 1, FKIND_BOOL = 2, FKIND_STRING = 3, FKIND_OTHER = 4 /* fixed width, null tests only */ };

struct FilterInsn {
  uint32_t op;       // FOP_*
  uint32_t cmp;      // ORCGPU_PRED_EQ .. _GE
  uint32_t col;      // index into the FilterCol table
  uint32_t lit_len;  // strings: bytes of the literal
  long long i;       // integer / Boolean literal
  double f;          // float literal
  unsigned long long lit_off;  // strings: where the literal starts in the literal pool
};

constexpr uint32_t kFilterStack = 64;  // = ORCGPU_FILTER_MAX_DEPTH: a predicate of depth d needs at most d slots of the evaluation stack
