// agg_program.h -- an aggregate list as the host compiles it (orcgpu_agg_plan.inc) and agg_partial_kernel / agg_final_kernel run
// it (agg_kernels.hip), and the record both kernels and the host's merge speak in.  Plain C++: no HIP in here.
#pragma once
#include <stddef.h>
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
  AK_N = 11,           // the kinds agg_partial_kernel / agg_group_partial_kernel reduce
  // SUM / AVG of an arithmetic expression: a program of AggExprOp per kept row (agg_expr_eval.h), reduced by kernels of their own
  // (agg_expr_partial_kernel / agg_group_expr_partial_kernel), so that the kinds above keep their registers.  col / col2 are the
  // program's offset and length in the op table uploaded beside the instructions, not column indexes.
  AK_EXPR_INT = 11,    // every value a signed 128-bit integer, the sum in 192 bits
  AK_EXPR_DEC = 12,    // ... the unscaled value of a Decimal at the root's scale
  AK_EXPR_F64 = 13,    // doubles, every operation rounded once
  AK_ALL_N = 14
};
enum { AGG_OVERFLOW = 1, AGG_SAW_NAN = 2 };
constexpr bool agg_is_expr(uint32_t kind) { return kind >= AK_EXPR_INT && kind < AK_ALL_N; }
// which of the two folds a kind takes: a float sum, a 192-bit sum (the counts are sums), or MIN / MAX
constexpr bool agg_is_float_sum(uint32_t kind) { return kind == AK_SUM_F64 || kind == AK_SP_F64 || kind == AK_EXPR_F64; }
constexpr bool agg_is_wide_sum(uint32_t kind) { return kind < AK_MINMAX_INT || kind == AK_EXPR_INT || kind == AK_EXPR_DEC; }

// One step of an expression's post-order program over at most kAggExprSlots operand slots.  A program begins with one AX_GATE per
// distinct column: a row in which one of them is NULL contributes nothing.
enum {
  AX_GATE = 0,       // col: the row counts only when this column's value is not NULL
  AX_PUSH_INT = 1,   // col (FKIND_INT): its int64, sign-extended
  AX_PUSH_DEC = 2,   // col (FKIND_DEC128): its unscaled 128-bit value
  AX_PUSH_F64 = 3,   // col (FKIND_FLOAT): its double, a Float32 widened first
  AX_PUSH_LIT = 4,   // lo / hi: a 128-bit integer, or in lo the bits of a double
  AX_ADD = 5,        // the two top slots a (below) and b (top) -> a + b
  AX_SUB = 6,        //                                          -> a - b
  AX_RSUB = 7,       //                                          -> b - a (the right child was evaluated first)
  AX_MUL = 8,        //                                          -> a * b
  AX_NEG = 9,        // the top slot -> its negation
  AX_SCALE10 = 10,   // the top slot -> itself times lo / hi = 10^k (k in `col`), exactly
  AX_DATE_PART = 11, // the top slot, days since 1970-01-01 -> a calendar field of that day (`col`: AX_PART_*); outside int32: overflow
  // Division (include/orcgpu.h: DIVISION).  Each takes the two top slots a (below) and b (top), like AX_SUB; none commutes, and there
  // are no reversed forms: where the right child was evaluated first, the compiler puts ONE AX_SWAP in front of the op.
  AX_DIV = 12,       // -> a / b.  INT / DEC: round(a * 10^k / b), half away from zero (k in `col`, 10^k in lo / hi); FLOAT: one IEEE division
  AX_FLOOR_DIV = 13, // -> floor(a / b), integers (INT / DEC alone)
  AX_MOD = 14,       // -> a - floor(a / b) * b: the remainder with the divisor's sign (INT / DEC alone)
  AX_SWAP = 15,      // the two top slots change places
  // Conditionals (include/orcgpu.h: CONDITIONALS).  A program that holds one of these has NO gates: every slot carries, beside its
  // value, a NULL bit and an overflow bit (agg_expr_eval.h: AggSlotBits), its column pushes are "nullable" (lo = 1: the slot's NULL
  // bit is the row's validity), and only the root's bits decide the row.  A condition is a slot like any other: 1 TRUE, 0 FALSE,
  // the NULL bit UNKNOWN.  Only the interpreter with the conditionals runs them: the host launches it for such a program, and the
  // program is marked so that any other interpreter overflows the row (kAggCondMark, below).
  AX_CMP = 16,       // the two top slots a (below) and b (top) -> a `col` b (`col`: 0 .. 5 for = != < <= > >=); UNKNOWN where either is NULL
  AX_IS_NULL = 17,   // the top slot -> TRUE where it is NULL, else FALSE: never UNKNOWN
  AX_AND = 18,       // the two top slots -> Kleene's AND; a FALSE operand decides, whatever the other one is or did
  AX_OR = 19,        //                   -> Kleene's OR; a TRUE operand decides
  AX_NOT = 20,       // the top slot -> Kleene's NOT
  AX_IF = 21,        // the three top slots -> the `then` slot where the condition is TRUE, else the `otherwise` slot, with the chosen
                     // slot's NULL and overflow bits.  The condition is always evaluated first and stands lowest; `col` = 0: then
                     // below otherwise, 1: otherwise was evaluated first and stands below then.  (The slots by NUMBER, any of the
                     // six orders, was tried: the select by a slot number put the slots into scratch memory.)
  AX_COALESCE = 22,  // the two top slots a (below) and b (top) -> a unless a is NULL, then b
  AX_ABS = 23,       // the top slot -> its magnitude; -2^127 overflows; a double: the sign bit cleared
  AX_PUSH_NULL = 24, // a slot whose NULL bit is set
  // Conversions (include/orcgpu.h: CONVERSIONS).  A program that holds one may hold values of BOTH kinds: a slot is 128 bits, and a
  // double lives as its bits in the slot's low word.  Only the mixed interpreter (agg_expr_eval.h: agg_expr_eval_mixed) runs them; such a
  // program is laid out like one with conditionals -- no gates, nullable pushes, NULL and overflow per slot -- behind a mark and in
  // front of a tail that make every other interpreter overflow the row or give NaN (kAggConvMarkCol, below).  Each takes the top slot.
  AX_TO_F64 = 25,      // an integer / the unscaled value of a Decimal at scale k -> the double nearest value / 10^k, ties to even
                       // (k in `col`, 10^k in lo / hi); never an overflow
  AX_F64_TO_DEC = 26,  // a double -> round(x * 10^t), half away from zero, computed exactly (t in `col`, 10^t in lo / hi); NaN, an
                       // infinity and a magnitude of 10^38 or more overflow
  AX_F64_TO_INT = 27,  // a double -> truncated toward zero; NaN, an infinity and a result outside int64 overflow
  AX_RESCALE = 28,     // an unscaled Decimal -> itself divided by 10^k (k in the low byte of `col`, 10^k in lo / hi), rounded by the
                       // mode in bits 8 .. 9 of `col` (AGG_ROUND_*): `col` has the room, no new field; never an overflow
  AX_FIT_I64 = 29,     // the value unchanged; outside int64: overflow
  AX_F64_ROUND = 30,   // a double -> round / floor / ceil / trunc of it (`col`: AGG_ROUND_*), still a double; NaN and infinities pass
  AX_N = 31
};
// The rounding modes of AX_RESCALE and AX_F64_ROUND
enum { AGG_ROUND_HALF_AWAY = 0, AGG_ROUND_FLOOR = 1, AGG_ROUND_CEIL = 2, AGG_ROUND_TRUNC = 3 };
// The calendar fields of AX_DATE_PART (include/orcgpu.h: ORCGPU_DATE_PART_*), proleptic Gregorian, astronomical year numbering
enum { AX_PART_YEAR = 0, AX_PART_QUARTER = 1, AX_PART_MONTH = 2, AX_PART_DAY = 3, AX_PART_DAY_OF_WEEK = 4, AX_PART_DAY_OF_YEAR = 5, AX_PART_N = 6 };
constexpr uint32_t kAggExprSlots = 4, kAggExprMaxNodes = 32;
struct AggExprOp {
  uint32_t op;   // AX_*
  uint32_t col;  // index into the FilterCol table; AX_SCALE10, AX_DIV, AX_TO_F64 ..: k; AX_DATE_PART: AX_PART_*; AX_CMP: the comparison; AX_IF: the slots
  unsigned long long lo, hi;  // (AX_PUSH_INT / _DEC / _F64: lo = 1 in a program with conditionals: the push is nullable)
};

// Does a table of programs hold a division?  The host asks before a launch: the kernels that interpret programs come in two
// instantiations, and the one without the divide keeps the registers -- and the occupancy -- it had before there was one.
inline bool agg_ops_hold_division(const AggExprOp* ops, size_t n) {
  for (size_t k = 0; k < n; k++)
    if (ops[k].op >= AX_DIV && ops[k].op <= AX_MOD) return true;
  return false;
}

// ... or a conditional?  (The same question for the third instantiation, the one with the divide AND the conditionals.)
inline bool agg_ops_hold_conditional(const AggExprOp* ops, size_t n) {
  for (size_t k = 0; k < n; k++)
    if (ops[k].op >= AX_CMP && ops[k].op <= AX_PUSH_NULL) return true;
  return false;
}
// AX_IF's `col`: which branch was evaluated first
constexpr uint32_t kAggIfThenFirst = 0, kAggIfElseFirst = 1;
// What makes a program with conditionals safe in the hands of an interpreter WITHOUT them, at no cost to that interpreter: existing
// ops.  Its first op is kAggCondMark, an AX_MOD, which no other program begins with (a binary op needs operands): over the empty,
// all-zero slots it is a division by zero -- or a division the instantiation lacks --, `ok` is sticky and the row overflows.  The
// double interpreter has no AX_MOD and no overflow; there the program ends with kAggCondTailF64 ops, `AX_PUSH_LIT NaN, AX_ADD`:
// whatever the ops it knows left on top, the result is NaN, as a division's is without the divide.  The interpreter with the
// conditionals skips the mark and the tail.
constexpr uint32_t kAggCondMark = AX_MOD, kAggCondTailF64 = 2;
constexpr unsigned long long kAggCondNaNBits = 0x7ff8000000000000ull;
constexpr bool agg_cond_marked(const AggExprOp* prog, uint32_t n) { return n != 0 && prog[0].op == kAggCondMark; }
// A program with conversions (AX_TO_F64 .. AX_F64_ROUND) gets the same protection, from the interpreters with the conditionals too
// -- they skip the mark -- and again at no cost to any of them: existing ops.  Its mark is the conditionals' with kAggConvMarkCol in
// `col` (no other AX_MOD has a `col`), and it ENDS with kAggConvTail ops that only the interpreters WITHOUT the conversions run:
//   a root of the INT / DEC class   push 0, push 0, AX_MOD (a slot that overflowed), AX_SWAP, AX_COALESCE: the overflowed slot is
//                                   not NULL, so it is the result -- the row overflows whatever the ops they know left on top;
//   a root of the FLOAT class       push NaN, AX_SWAP, AX_COALESCE (the interpreter with the conditionals: NaN, not NULL), then
//                                   kAggCondTailF64's push NaN, AX_ADD, which that interpreter strips and the plain one runs: NaN.
// The mixed interpreter skips the mark and the tail.
// In such a program an arithmetic op, AX_NEG, AX_ABS and AX_CMP say which kind their operands are: kAggOpF64 in `hi` -- the one bit
// no power of ten reaches (10^38 < 2^127) and no such op used.  (The alternative, float twins of those eleven ops, was not taken:
// the twins would double the interpreter's switch, where the flag is one test on an op already loaded.)
constexpr uint32_t kAggConvMarkCol = 1, kAggConvTail = 5;
constexpr unsigned long long kAggOpF64 = 1ull << 63;
constexpr bool agg_conv_marked(const AggExprOp* prog, uint32_t n) { return agg_cond_marked(prog, n) && prog[0].col == kAggConvMarkCol; }
// ... or a conversion?  (The fourth instantiation: the mixed interpreter.)  A program compiled with per-node classes is one even
// where folding left it no conversion op: its mark says so.
inline bool agg_ops_hold_conversion(const AggExprOp* ops, size_t n) {
  for (size_t k = 0; k < n; k++)
    if ((ops[k].op >= AX_TO_F64 && ops[k].op < AX_N) || (ops[k].op == kAggCondMark && ops[k].col == kAggConvMarkCol)) return true;
  return false;
}

struct AggInsn {
  uint32_t kind;     // AK_*
  uint32_t is_max;   // AK_MINMAX_*: 1 = MAX
  uint32_t col;      // index into the FilterCol table (AK_EXPR_*: the program's first op in the op table)
  uint32_t col2;     // AK_SP_*: the second operand (AK_EXPR_*: the program's length)
  uint32_t fkind;    // FKIND_* of `col` as the decode left it
  uint32_t op;       // ORCGPU_AGG_* as given
  int32_t scale;     // Decimal results: the scale; Timestamp MIN / MAX: the unit
  uint32_t cond;     // 0: every kept row; k + 1: the kept rows of condition plane k (KeptRows::cond) -- agg(x) FILTER (WHERE ...)
};
// Where the program of one distinct condition lies in the call's predicate program (FilterInsn, filter_program.h): what
// agg_cond_eval_kernel evaluates into plane blockIdx.y
struct AggCondSpan {
  uint32_t first, n;
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
