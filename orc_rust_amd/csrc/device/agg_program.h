// agg_program.h -- an aggregate list as the host compiles it (orcgpu_agg_plan.inc) and agg_partial_kernel / agg_final_kernel run
// it (agg_kernels.hip), and the record both kernels and the host's merge speak in.  Plain C++: no HIP in here.
#pragma once
#include <stdint.h>

// What an instruction accumulates, and from what the column holds (the FKIND_* of filter_program.h say how a value is loaded)
enum {
  AK_COUNT_ROWS = 0,   // kept rows
  AK_COUNT = 1,        // kept rows whose value is not null: the validity alone is read
  AK_SUM_INT = 2,      // int64 values, exact in 192 bits
  AK_SUM_DEC = 3,      // Decimal128 unscaled values, exact in 192 bits
  AK_SUM_F64 = 4,      // doubles (a Float32 widened first), in the fixed order of the reduction
  AK_SP_INT = 5,       // col * col2, each product exact in 128 bits, the sum in 192
  AK_SP_DEC = 6,       // ... of Decimal128 operands that fit a signed 64-bit word (one that does not: AGG_OVERFLOW, the row is left out)
  AK_SP_F64 = 7,       // ... of doubles, each product rounded once
  AK_MINMAX_INT = 8,   // int64 (integers, Date, Timestamp in its unit; FKIND_BOOL: the bit as 0 / 1)
  AK_MINMAX_DEC = 9,   // Decimal128, signed 128-bit order
  AK_MINMAX_F64 = 10,  // doubles; NaN values are left out and noted (AGG_SAW_NAN)
  AK_N = 11
};
enum { AGG_OVERFLOW = 1, AGG_SAW_NAN = 2 };

struct AggInsn {
  uint32_t kind;     // AK_*
  uint32_t is_max;   // AK_MINMAX_*: 1 = MAX
  uint32_t col;      // index into the FilterCol table
  uint32_t col2;     // AK_SP_*: the second operand
  uint32_t fkind;    // FKIND_* of `col` as the decode left it
  uint32_t op;       // ORCGPU_AGG_* as given
  int32_t scale;     // Decimal results: the scale; Timestamp MIN / MAX: the unit
  uint32_t pad;
};

// A partial result, and the final one: `count` values went into it (0: NULL for everything but the counts, which live in w[0]).
//   sums: w[0..2] a signed 192-bit integer, little-endian words, or f;  MIN / MAX: w[0] (int64), w[0..1] (int128) or f.
struct AggPartial {
  unsigned long long w[3];
  double f;
  unsigned long long count;
  uint32_t flags;  // AGG_*
  uint32_t pad;
};

// Blocks of agg_partial_kernel's grid along x: a function of the input row count alone, so that a float sum has one shape -- and
// one result, bit for bit -- per (rows, batch size).  Four wavefronts a block, a 64-row word of the keep mask per wavefront trip.
constexpr uint32_t kAggMaxBlocks = 1024;
inline uint32_t agg_blocks(uint64_t n_in) {
  const uint64_t n_words = (n_in + 63) / 64, b = (n_words + 3) / 4;
  return (uint32_t)(b < kAggMaxBlocks ? b : kAggMaxBlocks);
}
