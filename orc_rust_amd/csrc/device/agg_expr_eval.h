// agg_expr_eval.h -- the arithmetic of an aggregate's expression (include/orcgpu.h: ORCGPU_AGG_OP_SUM_EXPR / _AVG_EXPR), ONE text
// for the kernels (agg_kernels.hip), the host's plan compiler, which folds literals with it (orcgpu_agg_expr.inc), and the CPU
// check that runs it against Python ints (tests/hostcheck/agg_expr_check.cpp): checked signed 128-bit add / subtract / multiply /
// negate, the powers of ten, the interpreter of a program of AggExprOp (agg_program.h) over four operand slots, and -- host only --
// AVG's division.  Plain C++ behind AGG_HD; nothing wraps silently: an operation whose exact result does not fit a signed
// 128-bit integer reports it, and the caller sets AGG_OVERFLOW.  Division (/, //, %) is here too: a signed 128-by-128-bit divide
// by magnitudes with explicit paths, never the compiler's expansion of `__int128 /`; a zero divisor overflows the row.  So are the
// conversions between the classes (include/orcgpu.h: CONVERSIONS) and the mixed interpreter that runs a program holding values of
// both kinds (tests/hostcheck/conv_check.cpp).
#pragma once
#include <stdint.h>

#include "agg_program.h"

#if defined(__HIPCC__)
#define AGG_HD __host__ __device__ __forceinline__
#else
#define AGG_HD inline
#endif

typedef __int128 agg_i128;
typedef unsigned __int128 agg_u128;

AGG_HD agg_i128 agg_i128_of(unsigned long long lo, unsigned long long hi) { return (agg_i128)(((agg_u128)hi << 64) | lo); }
AGG_HD agg_i128 agg_i128_min() { return (agg_i128)((agg_u128)1 << 127); }

// r = a + b; false when the exact sum does not fit (r is then the wrapped value, not to be used)
AGG_HD bool agg_add_checked(agg_i128 a, agg_i128 b, agg_i128* r) {
  const agg_u128 s = (agg_u128)a + (agg_u128)b;
  *r = (agg_i128)s;
  return (agg_i128)(((agg_u128)a ^ s) & ((agg_u128)b ^ s)) >= 0;
}
AGG_HD bool agg_sub_checked(agg_i128 a, agg_i128 b, agg_i128* r) {
  const agg_u128 s = (agg_u128)a - (agg_u128)b;
  *r = (agg_i128)s;
  return (agg_i128)(((agg_u128)a ^ (agg_u128)b) & ((agg_u128)a ^ s)) >= 0;
}
AGG_HD bool agg_neg_checked(agg_i128 a, agg_i128* r) {
  *r = (agg_i128)((agg_u128)0 - (agg_u128)a);
  return a != agg_i128_min();
}
// r = a * b from the magnitudes' four 64 x 64 -> 128 partial products: the 256-bit product fits when its high half is zero and
// its low half is at most 2^127, 2^127 itself for a negative result only
AGG_HD bool agg_mul_checked(agg_i128 a, agg_i128 b, agg_i128* r) {
  const bool neg = (a < 0) != (b < 0);
  const agg_u128 ma = a < 0 ? (agg_u128)0 - (agg_u128)a : (agg_u128)a, mb = b < 0 ? (agg_u128)0 - (agg_u128)b : (agg_u128)b;
  const unsigned long long a0 = (unsigned long long)ma, a1 = (unsigned long long)(ma >> 64), b0 = (unsigned long long)mb, b1 = (unsigned long long)(mb >> 64);
  const agg_u128 p00 = (agg_u128)a0 * b0, p01 = (agg_u128)a0 * b1, p10 = (agg_u128)a1 * b0, p11 = (agg_u128)a1 * b1;
  // bits 64 .. 191: the cross products and the high word of p00; what passes bit 127 is the high half's
  const agg_u128 mid = (p00 >> 64) + (unsigned long long)p01 + (unsigned long long)p10;
  const bool high = p11 != 0 || (p01 >> 64) != 0 || (p10 >> 64) != 0 || (mid >> 64) != 0;
  const agg_u128 low = (mid << 64) | (unsigned long long)p00;
  const agg_u128 top = (agg_u128)1 << 127;
  *r = (agg_i128)(neg ? (agg_u128)0 - low : low);
  return !high && (low < top || (neg && low == top));
}
// 10^k, k = 0 .. 38 (what a Decimal128's 38 digits take)
AGG_HD agg_i128 agg_pow10(uint32_t k) {
  agg_i128 v = 1;
  for (uint32_t x = 0; x < k && x < 38; x++) v *= 10;
  return v;
}

// ---- division (include/orcgpu.h: DIVISION): by magnitudes, with explicit paths.  gfx950 divides nothing wider than 32 bits in one
// instruction; a 64-bit unsigned `/` is the widest the compiler is asked to expand here, and `__int128 /` is never written.

// (u1 : u0) / v for u1 < v, so that the quotient fits 64 bits; *rem gets the remainder.  Knuth's algorithm D in two digits of 32
// bits: v normalised, each quotient digit estimated from the divisor's top digit and corrected at most twice.
AGG_HD unsigned long long agg_div128_u64(unsigned long long u1, unsigned long long u0, unsigned long long v, unsigned long long* rem) {
  const unsigned long long b = 1ull << 32;
  const int s = __builtin_clzll(v);  // (v != 0: u1 < v)
  v <<= s;
  const unsigned long long vn1 = v >> 32, vn0 = v & 0xffffffffull;
  const unsigned long long un32 = s ? (u1 << s) | (u0 >> (64 - s)) : u1, un10 = u0 << s;
  const unsigned long long un1 = un10 >> 32, un0 = un10 & 0xffffffffull;
  unsigned long long q1 = un32 / vn1, rhat = un32 - q1 * vn1;
  for (int k = 0; k < 2 && rhat < b && (q1 >= b || q1 * vn0 > (rhat << 32 | un1)); k++) {
    q1--;
    rhat += vn1;
  }
  const unsigned long long un21 = (un32 << 32 | un1) - q1 * v;  // (modulo 2^64: the true value is below v)
  unsigned long long q0 = un21 / vn1;
  rhat = un21 - q0 * vn1;
  for (int k = 0; k < 2 && rhat < b && (q0 >= b || q0 * vn0 > (rhat << 32 | un0)); k++) {
    q0--;
    rhat += vn1;
  }
  *rem = ((un21 << 32 | un0) - q0 * v) >> s;
  return (q1 << 32) + q0;
}

// n / d of unsigned 128-bit magnitudes, d != 0; *rem gets the remainder.  Three paths, chosen per lane:
//   both below 2^64 (almost every real row)   one 64-bit unsigned divide
//   d below 2^64, n not                       long division, a 128-by-64 step per word of n
//   d of 2^64 or more                         the quotient is below 2^64: estimated from the divisor's top 64 normalised bits over
//                                             n / 2 (at most one too large once shifted back, so one is taken off), corrected once
AGG_HD agg_u128 agg_udivmod128(agg_u128 n, agg_u128 d, agg_u128* rem) {
  const unsigned long long n0 = (unsigned long long)n, n1 = (unsigned long long)(n >> 64), d0 = (unsigned long long)d, d1 = (unsigned long long)(d >> 64);
  if (d1 == 0) {
    if (n1 == 0) {
      const unsigned long long q = n0 / d0;
      *rem = n0 - q * d0;
      return q;
    }
    const unsigned long long q1 = n1 / d0;
    unsigned long long r = n1 - q1 * d0;
    const unsigned long long q0 = agg_div128_u64(r, n0, d0, &r);
    *rem = r;
    return ((agg_u128)q1 << 64) | q0;
  }
  const int s = __builtin_clzll(d1);
  const unsigned long long v1 = (unsigned long long)((d << s) >> 64);  // bit 63 is set
  unsigned long long r = 0;
  unsigned long long q = agg_div128_u64(n1 >> 1, (n1 << 63) | (n0 >> 1), v1, &r) >> (63 - s);  // (n1 / 2 < 2^63 <= v1)
  if (q) q--;
  agg_u128 left = n - ((agg_u128)q * d0 + ((agg_u128)(q * d1) << 64));  // q * d <= n: nothing leaves 128 bits
  if (left >= d) {
    q++;
    left -= d;
  }
  *rem = left;
  return q;
}

enum { AGG_DIV_ROUND = 0, AGG_DIV_FLOOR = 1, AGG_DIV_MOD = 2 };
static_assert(AX_FLOOR_DIV - AX_DIV == AGG_DIV_FLOOR && AX_MOD - AX_DIV == AGG_DIV_MOD, "the interpreter takes the mode off the op");
// The three divisions of two signed 128-bit integers: AGG_DIV_ROUND the exact quotient rounded half away from zero (a Decimal
// division, its dividend already times 10^k), AGG_DIV_FLOOR the floored quotient and AGG_DIV_MOD the remainder that goes with it
// (the divisor's sign, as Python and numpy have them: a == (a // b) * b + a % b).  The magnitudes are divided, then the rounding or
// the floor adjustment applied, then the sign.  false, and *r = 0: b is zero, or the quotient is 2^127 (-2^127 by -1).
AGG_HD bool agg_div_checked(agg_i128 a, agg_i128 b, uint32_t mode, agg_i128* r) {
  *r = 0;
  if (b == 0) return false;
  const bool neg = (a < 0) != (b < 0);
  const agg_u128 ma = a < 0 ? (agg_u128)0 - (agg_u128)a : (agg_u128)a, mb = b < 0 ? (agg_u128)0 - (agg_u128)b : (agg_u128)b;
  agg_u128 rem = 0;
  agg_u128 q = agg_udivmod128(ma, mb, &rem);
  if (mode == AGG_DIV_MOD) {
    const agg_u128 m = neg && rem != 0 ? mb - rem : rem;  // below |b|: it fits
    *r = (agg_i128)(b < 0 ? (agg_u128)0 - m : m);
    return true;
  }
  // half or more away from zero (rem < mb: no carry in mb - rem; a quotient that is bumped is below 2^127); the floor of a
  // negative inexact quotient is one further from zero
  if (mode == AGG_DIV_ROUND ? rem >= mb - rem : neg && rem != 0) q++;
  const agg_u128 top = (agg_u128)1 << 127;
  if (q > top || (q == top && !neg)) return false;
  *r = (agg_i128)(neg ? (agg_u128)0 - q : q);
  return true;
}
// a / b of Decimals: round(a * 10^k / b) with `pow` = 10^k.  false: b is zero, a * 10^k leaves 128 bits, or the quotient does.
AGG_HD bool agg_div_scaled_checked(agg_i128 a, agg_i128 pow, agg_i128 b, agg_i128* r) {
  agg_i128 n = 0;
  *r = 0;
  return agg_mul_checked(a, pow, &n) && agg_div_checked(n, b, AGG_DIV_ROUND, r);
}

// A calendar field (AX_PART_*) of the day `days` after 1970-01-01, proleptic Gregorian with astronomical year numbering (year 0
// exists, the years before it are negative), for every int32: civil-from-days by the 400-year era.  32-bit unsigned arithmetic
// throughout, so that every division is by a constant and becomes a multiply-high; no table, no loop over years.
// FLOOR, not C's truncation, for the days before the era's origin: the day number is first moved to where nothing is negative.
// n = days + 2^31 counts from day -2^31; that day lies kDateEra0 whole eras and kDateDay0 days after a 1 March of a year divisible
// by 400 (0000-03-01 is day -719468, and -2^31 + 719468 = -14695 * 146097 + 131235).  n / 146097 and n % 146097 are taken of the
// unsigned n, the kDateDay0 days are added to the remainder -- one conditional carry into the era -- and the era number is made
// signed again at the end, in the year alone.
constexpr uint32_t kDateEraDays = 146097, kDateDay0 = 131235;
constexpr int32_t kDateEra0 = -14695;
static_assert((long long)kDateEra0 * kDateEraDays + kDateDay0 == -2147483648LL + 719468, "day -2^31 in eras and days since 0000-03-01");
AGG_HD int32_t agg_date_part(int32_t days, uint32_t part) {
  const uint32_t n = (uint32_t)days ^ 0x80000000u;  // days + 2^31, 0 .. 2^32 - 1
  if (part == AX_PART_DAY_OF_WEEK) {  // ISO, Monday = 1: 1970-01-01 is a Thursday, and 2^31 = 2 (mod 7), so n = days + 2 (mod 7)
    const uint32_t w = n % 7u + 1u;   // days + 3 (mod 7), 1 .. 7: 0 = Monday
    return (int32_t)((w >= 7u ? w - 7u : w) + 1u);
  }
  uint32_t era = n / kDateEraDays, doe = n - era * kDateEraDays + kDateDay0;  // doe: the day of the era, 0 .. 146096 after the carry
  if (doe >= kDateEraDays) {
    doe -= kDateEraDays;
    era++;
  }
  // the era's four centuries of 36524 days (the last one a day longer), a century's 25 groups of four years of 1461 days (the last
  // one of a short century a day shorter), a group's four years of 365 days (the last one a day longer): a quotient of 4 is the
  // last day of the longer last part
  uint32_t cent = doe / 36524u;
  cent -= cent >> 2;
  const uint32_t doc = doe - cent * 36524u;  // 0 .. 36524
  const uint32_t quad = doc / 1461u;         // 0 .. 24
  const uint32_t doq = doc - quad * 1461u;   // 0 .. 1460
  uint32_t yoq = doq / 365u;
  yoq -= yoq >> 2;
  const uint32_t doy = doq - yoq * 365u;  // the day of the year that begins on 1 March, 0 .. 365
  const uint32_t mp = (5u * doy + 2u) / 153u;  // its month, 0 = March .. 11 = February
  const uint32_t month = mp < 10u ? mp + 3u : mp - 9u;
  if (part == AX_PART_MONTH) return (int32_t)month;
  if (part == AX_PART_QUARTER) return (int32_t)((month + 2u) / 3u);
  if (part == AX_PART_DAY) return (int32_t)(doy - (153u * mp + 2u) / 5u + 1u);
  if (part == AX_PART_DAY_OF_YEAR) {
    // January and February close the March year: day 306 is 1 January.  From March on, the civil year is the March year, a leap
    // year when it is the first of its group of four -- but not the first of a century, unless of the era
    const uint32_t leap = (yoq == 0u && (quad != 0u || cent == 0u)) ? 1u : 0u;
    return (int32_t)(mp < 10u ? doy + 60u + leap : doy - 305u);
  }
  return (kDateEra0 + (int32_t)era) * 400 + (int32_t)(cent * 100u + quad * 4u + yoq) + (month <= 2u ? 1 : 0);  // AX_PART_YEAR
}

// (contraction is switched off for the evaluator by name: the rounded-operation intrinsics alone are plain + and * in some
// toolchains, and "one IEEE operation" must not rest on where the optimiser happens to see a multiply and an add)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
AGG_HD double agg_f64_add(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dadd_rn(a, b);
#else
  volatile double r = a + b;  // (one rounding: nothing to contract with)
  return r;
#endif
}
AGG_HD double agg_f64_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, b);  // never contracted into an FMA with the addition behind it
#else
  volatile double r = a * b;
  return r;
#endif
}
AGG_HD double agg_f64_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ddiv_rn(a, b);  // correctly rounded; x / 0 is an infinity and 0 / 0 NaN, as IEEE says
#else
  volatile double r = a / b;
  return r;
#endif
}
AGG_HD double agg_f64_of_bits(unsigned long long u) {
  union {
    unsigned long long u;
    double d;
  } x;
  x.u = u;
  return x.d;
}
AGG_HD unsigned long long agg_bits_of_f64(double d) {
  union {
    unsigned long long u;
    double d;
  } x;
  x.d = d;
  return x.u;
}

// The four operand slots as named values, moved on push and pop: s0 is the top.  (An indexed private array would live in scratch
// memory on the GPU.)
template <typename T>
struct AggSlots {
  T s0, s1, s2, s3;
  AGG_HD void push(T v) {
    s3 = s2;
    s2 = s1;
    s1 = s0;
    s0 = v;
  }
  // the two top slots -> one: what stood below them moves up
  AGG_HD void merge(T v) {
    s0 = v;
    s1 = s2;
    s2 = s3;
  }
  AGG_HD void swap() {
    const T v = s0;
    s0 = s1;
    s1 = v;
  }
  // the three top slots -> one (AX_IF)
  AGG_HD void merge3(T v) {
    s0 = v;
    s1 = s3;
  }
};

// What the interpreter with the conditionals (include/orcgpu.h: CONDITIONALS) knows of each slot beside its value: whether it is
// NULL and whether it overflowed, as two masks -- bit k is slot k, bit 0 the top -- moved as AggSlots moves the values.  Two words,
// not an array: no scratch.  A slot never has both bits: where an operand is NULL the result is NULL, overflow or not.
struct AggSlotBits {
  uint32_t nul, ovf;
  AGG_HD bool n(uint32_t k) const { return (nul >> k) & 1; }
  AGG_HD bool o(uint32_t k) const { return (ovf >> k) & 1; }
  AGG_HD void push(bool n_, bool o_) {
    nul = ((nul << 1) | (n_ ? 1u : 0u)) & 15u;
    ovf = ((ovf << 1) | (o_ ? 1u : 0u)) & 15u;
  }
  AGG_HD void set(bool n_, bool o_) {
    nul = (nul & ~1u) | (n_ ? 1u : 0u);
    ovf = (ovf & ~1u) | (o_ ? 1u : 0u);
  }
  AGG_HD void merge(bool n_, bool o_) {
    nul = ((nul >> 2) << 1) | (n_ ? 1u : 0u);
    ovf = ((ovf >> 2) << 1) | (o_ ? 1u : 0u);
  }
  AGG_HD void merge3(bool n_, bool o_) {
    nul = ((nul >> 3) << 1) | (n_ ? 1u : 0u);
    ovf = ((ovf >> 3) << 1) | (o_ ? 1u : 0u);
  }
  AGG_HD void swap() {
    nul = (nul & ~3u) | ((nul & 1u) << 1) | ((nul >> 1) & 1u);
    ovf = (ovf & ~3u) | ((ovf & 1u) << 1) | ((ovf >> 1) & 1u);
  }
};

enum { AGG_ROW_NULL = 0, AGG_ROW_VALUE = 1, AGG_ROW_OVERFLOW = 2 };

// Kleene's AND (is_or = false) / OR of two conditions, each a value (non-zero: TRUE), a NULL bit (UNKNOWN) and an overflow bit.  The
// operand that decides -- a known FALSE under AND, a known TRUE under OR -- decides whatever the other one is: that is what makes
// `b != 0 AND a / b > 2` a guard.  Otherwise overflow comes before UNKNOWN.
AGG_HD void agg_kleene(bool is_or, bool va, bool na, bool oa, bool vb, bool nb, bool ob, bool* v, bool* n, bool* o) {
  const bool decided = (!na && !oa && va == is_or) || (!nb && !ob && vb == is_or);
  *o = !decided && (oa || ob);
  *n = !decided && !*o && (na || nb);
  *v = decided ? is_or : !is_or;  // (neither decides and both are known: TRUE AND TRUE, FALSE OR FALSE)
}
// a `cmp` b from "a < b" and "a == b" (for doubles: IEEE's, both false with a NaN -- then only != holds)
AGG_HD bool agg_cmp_of(uint32_t cmp, bool lt, bool eq, bool gt) {
  return cmp == 0 ? eq : cmp == 1 ? !eq : cmp == 2 ? lt : cmp == 3 ? (lt || eq) : cmp == 4 ? gt : (gt || eq);
}

// ---- conversions (include/orcgpu.h: CONVERSIONS): between the classes, and rounding inside them.  Integer code throughout but for
// the one division of the fast path and the four IEEE roundings; no table, no indexed array.

AGG_HD int agg_bits_u128(agg_u128 v) {
  const unsigned long long hi = (unsigned long long)(v >> 64), lo = (unsigned long long)v;
  return hi ? 128 - __builtin_clzll(hi) : lo ? 64 - __builtin_clzll(lo) : 0;
}
AGG_HD agg_i128 agg_pow10_38() { return agg_i128_of(0x098a224000000000ull, 0x4b3b4ca85a86c47aull); }

// The double nearest the exact rational v / 10^k (`pow` = 10^k, k = 0 .. 38), ties to even: Python's float(Fraction(v, 10**k)).
// |v| < 2^53 and k <= 22: both are exact doubles, and one IEEE division of them is correctly rounded.  Otherwise the magnitudes
// are divided (agg_udivmod128), the remainder is extended bit by bit until the quotient has 56 significant bits -- where the
// quotient is 0 the remainder is first moved up by the zero bits that can only follow --, what is left is the sticky bit, and the
// rounding to 53 bits is done by hand.  The result lies in 10^-38 .. 2^127: never a subnormal, never an infinity.
AGG_HD double agg_to_f64(agg_i128 v, uint32_t k, agg_i128 pow) {
  if (v == 0) return 0.0;
  const bool neg = v < 0;
  const agg_u128 m = neg ? (agg_u128)0 - (agg_u128)v : (agg_u128)v, d = (agg_u128)pow;
  if (m < ((agg_u128)1 << 53) && k <= 22) {
    // (10^22 = 5^22 * 2^22 passes 64 bits: its two words are exact doubles, and so is their sum)
    const double dd = agg_f64_add(agg_f64_mul((double)(unsigned long long)(d >> 64), 18446744073709551616.0), (double)(unsigned long long)d);
    const double r = agg_f64_div((double)(unsigned long long)m, dd);
    return neg ? -r : r;
  }
  agg_u128 r = 0;
  agg_u128 q = agg_udivmod128(m, d, &r);
  int e = 0;  // the value is (q + r / d) * 2^e
  if (q == 0) {
    const int s = agg_bits_u128(d) - agg_bits_u128(m) - 1;  // (m < d: m << s has a bit less than d, it stays below it)
    if (s > 0) {
      r <<= s;
      e = -s;
    }
  }
  while (q < ((agg_u128)1 << 55)) {  // (r < d < 2^127: r << 1 fits)
    r <<= 1;
    const bool bit = r >= d;
    if (bit) r -= d;
    q = (q << 1) | (bit ? 1u : 0u);
    e--;
  }
  const int drop = agg_bits_u128(q) - 53;  // (at least 3)
  unsigned long long mant = (unsigned long long)(q >> drop);
  const agg_u128 rest = q & (((agg_u128)1 << drop) - 1), half = (agg_u128)1 << (drop - 1);
  if (rest > half || (rest == half && (r != 0 || (mant & 1)))) mant++;
  int ex = drop + e;  // mant * 2^ex
  if (mant >> 53) {
    mant >>= 1;
    ex++;
  }
  return agg_f64_of_bits(((unsigned long long)(1023 + 52 + ex) << 52) | (mant & ((1ull << 52) - 1)) | (neg ? 1ull << 63 : 0ull));
}

// round(x * 10^t), half away from zero, of the double's exact value m * 2^e (`pow` = 10^t): m (53 bits) times 10^t (at most 127)
// is held in three 64-bit words and shifted.  false, and *r = 0: NaN, an infinity, or a magnitude of 10^38 or more.  -0.0 gives 0.
AGG_HD bool agg_f64_to_dec(double x, agg_i128 pow, agg_i128* r) {
  *r = 0;
  const unsigned long long b = agg_bits_of_f64(x);
  const bool neg = (b >> 63) != 0;
  const uint32_t be = (uint32_t)(b >> 52) & 0x7ffu;
  unsigned long long m = b & ((1ull << 52) - 1);
  if (be == 0x7ffu) return false;
  int e = -1074;
  if (be != 0) {
    m |= 1ull << 52;
    e = (int)be - 1075;
  }
  if (m == 0) return true;
  const agg_u128 p = (agg_u128)pow;
  const agg_u128 lo = (agg_u128)(unsigned long long)p * m, hi = (agg_u128)(unsigned long long)(p >> 64) * m + (unsigned long long)(lo >> 64);
  unsigned long long w0 = (unsigned long long)lo, w1 = (unsigned long long)hi, w2 = (unsigned long long)(hi >> 64);
  agg_u128 q;
  if (e >= 0) {
    q = ((agg_u128)w1 << 64) | w0;
    if (w2 != 0 || e > 127 || agg_bits_u128(q) + e > 127) return false;  // (2^127 or more)
    q <<= e;
  } else {
    int sh = -e - 1;            // down to the bit behind the point: 0 .. 1073
    if (sh > 191) return true;  // (the product is below 2^180: less than a half)
    if (sh >= 128) {
      w0 = w2;
      w1 = 0;
      w2 = 0;
      sh -= 128;
    } else if (sh >= 64) {
      w0 = w1;
      w1 = w2;
      w2 = 0;
      sh -= 64;
    }
    if (sh) {
      w0 = (w0 >> sh) | (w1 << (64 - sh));
      w1 = (w1 >> sh) | (w2 << (64 - sh));
      w2 >>= sh;
    }
    if (w2 != 0) return false;  // (2^127 or more)
    q = ((agg_u128)w1 << 64) | w0;
    q = (q >> 1) + (unsigned long long)(q & 1);  // the bit behind the point is a half or more: away from zero
  }
  if (q >= (agg_u128)agg_pow10_38()) return false;
  *r = (agg_i128)(neg ? (agg_u128)0 - q : q);
  return true;
}
// x truncated toward zero.  false, and *r = 0: NaN, an infinity, or a result outside int64.
AGG_HD bool agg_f64_to_i64(double x, agg_i128* r) {
  *r = 0;
  if (!(x >= -9223372036854775808.0 && x < 9223372036854775808.0)) return false;
  *r = (agg_i128)(long long)x;
  return true;
}
// v / 10^k (`pow` = 10^k, k >= 1) to an integer by `mode` (AGG_ROUND_*): the magnitudes divided, then the mode, then the sign
AGG_HD agg_i128 agg_rescale(agg_i128 v, agg_i128 pow, uint32_t mode) {
  const bool neg = v < 0;
  const agg_u128 m = neg ? (agg_u128)0 - (agg_u128)v : (agg_u128)v, d = (agg_u128)pow;
  agg_u128 rem = 0;
  agg_u128 q = agg_udivmod128(m, d, &rem);
  const bool up = mode == AGG_ROUND_HALF_AWAY ? rem >= d - rem : mode == AGG_ROUND_FLOOR ? (neg && rem != 0) : mode == AGG_ROUND_CEIL ? (!neg && rem != 0) : false;
  if (up) q++;
  return (agg_i128)(neg ? (agg_u128)0 - q : q);
}
// C's round (half away from zero), floor, ceil, trunc: one IEEE operation each
AGG_HD double agg_f64_round(double x, uint32_t mode) {
  return mode == AGG_ROUND_HALF_AWAY ? __builtin_round(x) : mode == AGG_ROUND_FLOOR ? __builtin_floor(x) : mode == AGG_ROUND_CEIL ? __builtin_ceil(x) : __builtin_trunc(x);
}

// The MIXED interpreter: a program with conversions (agg_program.h: AX_TO_F64 .. AX_F64_ROUND) on one row.  A slot is 128 bits; an
// integer or an unscaled Decimal fills it, a double lives as its bits in the low word.  It is the interpreter with the divide and
// the conditionals (below) and more: NULL and overflow per slot (AggSlotBits), no jump, no indexed private array -- no scratch.  In
// a program with conversions an arithmetic op, AX_NEG, AX_ABS and AX_CMP carry kAggOpF64 where their operands are doubles; the kernels'
// fourth instantiation runs EVERY program of its launch here, so a program without conversions says by `f64cls` what all its
// operands are, and its mark and tail (kAggCondMark) are skipped as its own interpreter skips them.  A condition is the integer 1 / 0.
// Row: `valid`, `load_int`, `load_dec` and `load_f64`.  *out: the root's slot -- of the FLOAT class: the bits of the double.
template <typename Row>
AGG_HD int agg_expr_eval_mixed(const AggExprOp* prog, uint32_t n, const Row& row, bool f64cls, agg_i128* out) {
  AggSlots<agg_i128> s = {0, 0, 0, 0};
  AggSlotBits m = {0, 0};
  const bool marked = agg_cond_marked(prog, n), conv = agg_conv_marked(prog, n);
  const uint32_t tail = conv ? kAggConvTail : marked && f64cls ? kAggCondTailF64 : 0;
  n = n >= 1 + tail ? n - tail : marked ? 1 : n;
  for (uint32_t k = marked ? 1 : 0; k < n; k++) {
    const AggExprOp op = prog[k];
    const bool isf = conv ? (op.hi & kAggOpF64) != 0 : f64cls;
    agg_i128 r = 0;
    bool ok = true;
    switch (op.op) {
      case AX_GATE:
        if (!row.valid(op.col)) return AGG_ROW_NULL;
        break;
      case AX_PUSH_INT:
      case AX_PUSH_DEC:
      case AX_PUSH_F64: {
        const bool v = !op.lo || row.valid(op.col);
        if (v) r = op.op == AX_PUSH_INT ? row.load_int(op.col) : op.op == AX_PUSH_DEC ? row.load_dec(op.col) : (agg_i128)agg_bits_of_f64(row.load_f64(op.col));
        s.push(r);
        m.push(!v, false);
        break;
      }
      case AX_PUSH_LIT:
        s.push(agg_i128_of(op.lo, op.hi));
        m.push(false, false);
        break;
      case AX_PUSH_NULL:
        s.push(0);
        m.push(true, false);
        break;
      case AX_ADD:
      case AX_SUB:
      case AX_RSUB:
      case AX_MUL:
      case AX_DIV:
      case AX_FLOOR_DIV:
      case AX_MOD: {
        if (isf) {
          const double a = agg_f64_of_bits((unsigned long long)s.s1), b = agg_f64_of_bits((unsigned long long)s.s0);
          const double f = op.op == AX_ADD ? agg_f64_add(a, b) : op.op == AX_SUB ? agg_f64_add(a, -b) : op.op == AX_RSUB ? agg_f64_add(b, -a)
                         : op.op == AX_MUL ? agg_f64_mul(a, b) : agg_f64_div(a, b);
          r = (agg_i128)agg_bits_of_f64(f);
          ok = op.op <= AX_DIV;  // (// and % take no doubles: the compiler emits none)
        } else if (op.op == AX_ADD) {
          ok = agg_add_checked(s.s1, s.s0, &r);
        } else if (op.op == AX_SUB) {
          ok = agg_sub_checked(s.s1, s.s0, &r);
        } else if (op.op == AX_RSUB) {
          ok = agg_sub_checked(s.s0, s.s1, &r);
        } else if (op.op == AX_MUL) {
          ok = agg_mul_checked(s.s1, s.s0, &r);
        } else {
          agg_i128 a = s.s1;
          if (op.op == AX_DIV && op.col != 0) ok = agg_mul_checked(a, agg_i128_of(op.lo, op.hi & ~kAggOpF64), &a);
          ok &= agg_div_checked(a, s.s0, op.op - AX_DIV, &r);
        }
        const bool nul = m.n(0) || m.n(1);
        const bool ovf = !nul && (m.o(0) || m.o(1) || !ok);
        s.merge(nul || ovf ? (agg_i128)0 : r);
        m.merge(nul, ovf);
        break;
      }
      case AX_NEG:
      case AX_SCALE10:
      case AX_DATE_PART:
      case AX_ABS:
      case AX_TO_F64:
      case AX_F64_TO_DEC:
      case AX_F64_TO_INT:
      case AX_RESCALE:
      case AX_FIT_I64:
      case AX_F64_ROUND: {
        const unsigned long long bits = (unsigned long long)s.s0;
        const agg_i128 pow = agg_i128_of(op.lo, op.hi & ~kAggOpF64);
        if (op.op == AX_NEG) {
          if (isf) r = (agg_i128)(bits ^ (1ull << 63));
          else ok = agg_neg_checked(s.s0, &r);
        } else if (op.op == AX_SCALE10) {
          ok = agg_mul_checked(s.s0, pow, &r);
        } else if (op.op == AX_ABS) {
          r = s.s0;
          if (isf) r = (agg_i128)(bits & 0x7fffffffffffffffull);
          else if (r < 0) ok = agg_neg_checked(s.s0, &r);
        } else if (op.op == AX_DATE_PART) {
          const long long d = (long long)s.s0;
          ok = s.s0 == (agg_i128)(int32_t)d;
          r = (agg_i128)agg_date_part((int32_t)d, op.col);
        } else if (op.op == AX_TO_F64) {
          r = (agg_i128)agg_bits_of_f64(agg_to_f64(s.s0, op.col, pow));
        } else if (op.op == AX_F64_TO_DEC) {
          ok = agg_f64_to_dec(agg_f64_of_bits(bits), pow, &r);
        } else if (op.op == AX_F64_TO_INT) {
          ok = agg_f64_to_i64(agg_f64_of_bits(bits), &r);
        } else if (op.op == AX_RESCALE) {
          r = agg_rescale(s.s0, pow, (op.col >> 8) & 3u);
        } else if (op.op == AX_FIT_I64) {
          r = s.s0;
          ok = r == (agg_i128)(long long)r;
        } else {
          r = (agg_i128)agg_bits_of_f64(agg_f64_round(agg_f64_of_bits(bits), op.col & 3u));
        }
        const bool nul = m.n(0);
        const bool ovf = !nul && (m.o(0) || !ok);
        s.s0 = nul || ovf ? (agg_i128)0 : r;
        m.set(nul, ovf);
        break;
      }
      case AX_CMP: {
        const bool nul = m.n(0) || m.n(1);
        const bool ovf = !nul && (m.o(0) || m.o(1));
        bool lt = s.s1 < s.s0, eq = s.s1 == s.s0, gt = s.s1 > s.s0;
        if (isf) {
          const double a = agg_f64_of_bits((unsigned long long)s.s1), b = agg_f64_of_bits((unsigned long long)s.s0);
          lt = a < b;
          eq = a == b;
          gt = a > b;
        }
        const bool t = !nul && !ovf && agg_cmp_of(op.col, lt, eq, gt);
        s.merge(t ? 1 : 0);
        m.merge(nul, ovf);
        break;
      }
      case AX_IS_NULL:
        s.s0 = m.n(0) ? 1 : 0;
        m.set(false, m.o(0));
        break;
      case AX_AND:
      case AX_OR: {
        bool v, nul, ovf;
        agg_kleene(op.op == AX_OR, s.s1 != 0, m.n(1), m.o(1), s.s0 != 0, m.n(0), m.o(0), &v, &nul, &ovf);
        s.merge(v && !nul && !ovf ? 1 : 0);
        m.merge(nul, ovf);
        break;
      }
      case AX_NOT:
        s.s0 = !m.n(0) && !m.o(0) && s.s0 == 0 ? 1 : 0;
        break;
      case AX_IF: {
        const bool take = !m.n(2) && !m.o(2) && s.s2 != 0;
        const uint32_t at = take != (op.col != 0) ? 1u : 0u;
        const bool co = m.o(2);
        const bool nul = !co && m.n(at), ovf = co || m.o(at);
        r = nul || ovf ? (agg_i128)0 : (at ? s.s1 : s.s0);
        s.merge3(r);
        m.merge3(nul, ovf);
        break;
      }
      case AX_COALESCE: {
        const bool b = m.n(1);
        r = b ? s.s0 : s.s1;
        const bool nul = b ? m.n(0) : false, ovf = b ? m.o(0) : m.o(1);
        s.merge(r);
        m.merge(nul, ovf);
        break;
      }
      case AX_SWAP:
        s.swap();
        m.swap();
        break;
      default: break;
    }
  }
  *out = s.s0;
  return m.n(0) ? AGG_ROW_NULL : m.o(0) ? AGG_ROW_OVERFLOW : AGG_ROW_VALUE;
}

// A program WITH conditionals (agg_program.h: AX_CMP .. AX_PUSH_NULL) of the INT / DEC class on one row: no gates; every slot has
// its NULL and overflow bits, arithmetic hands them on (NULL first, then overflow), AX_IF and AX_COALESCE take the chosen slot's, and
// only the root's decide the row -- an untaken branch neither gates the row nor counts as an overflow.  Both branches are
// evaluated; there is no jump.
template <bool DIV, typename Row>
AGG_HD int agg_expr_eval_i128_cond(const AggExprOp* prog, uint32_t n, const Row& row, agg_i128* out) {
  AggSlots<agg_i128> s = {0, 0, 0, 0};
  AggSlotBits m = {0, 0};
  // (the mark in front of a program with conditionals -- agg_program.h: kAggCondMark -- is for the other interpreters: skipped)
  for (uint32_t k = agg_cond_marked(prog, n) ? 1 : 0; k < n; k++) {
    const AggExprOp op = prog[k];
    agg_i128 r = 0;
    bool ok = true;
    switch (op.op) {
      case AX_GATE:
        if (!row.valid(op.col)) return AGG_ROW_NULL;
        break;
      case AX_PUSH_INT:
      case AX_PUSH_DEC: {
        const bool v = !op.lo || row.valid(op.col);
        if (v) r = op.op == AX_PUSH_INT ? row.load_int(op.col) : row.load_dec(op.col);
        s.push(r);
        m.push(!v, false);
        break;
      }
      case AX_PUSH_LIT:
        s.push(agg_i128_of(op.lo, op.hi));
        m.push(false, false);
        break;
      case AX_PUSH_NULL:
        s.push(0);
        m.push(true, false);
        break;
      case AX_ADD:
      case AX_SUB:
      case AX_RSUB:
      case AX_MUL:
      case AX_DIV:
      case AX_FLOOR_DIV:
      case AX_MOD: {
        if (op.op == AX_ADD) {
          ok = agg_add_checked(s.s1, s.s0, &r);
        } else if (op.op == AX_SUB) {
          ok = agg_sub_checked(s.s1, s.s0, &r);
        } else if (op.op == AX_RSUB) {
          ok = agg_sub_checked(s.s0, s.s1, &r);
        } else if (op.op == AX_MUL) {
          ok = agg_mul_checked(s.s1, s.s0, &r);
        } else if constexpr (DIV) {
          agg_i128 a = s.s1;
          if (op.op == AX_DIV && op.col != 0) ok = agg_mul_checked(a, agg_i128_of(op.lo, op.hi), &a);
          ok &= agg_div_checked(a, s.s0, op.op - AX_DIV, &r);
        } else {
          ok = false;
        }
        const bool nul = m.n(0) || m.n(1);
        const bool ovf = !nul && (m.o(0) || m.o(1) || !ok);
        s.merge(nul || ovf ? (agg_i128)0 : r);
        m.merge(nul, ovf);
        break;
      }
      case AX_NEG:
      case AX_SCALE10:
      case AX_DATE_PART:
      case AX_ABS: {
        if (op.op == AX_NEG) {
          ok = agg_neg_checked(s.s0, &r);
        } else if (op.op == AX_SCALE10) {
          ok = agg_mul_checked(s.s0, agg_i128_of(op.lo, op.hi), &r);
        } else if (op.op == AX_ABS) {
          r = s.s0;
          if (r < 0) ok = agg_neg_checked(s.s0, &r);
        } else {
          const long long d = (long long)s.s0;
          ok = s.s0 == (agg_i128)(int32_t)d;
          r = (agg_i128)agg_date_part((int32_t)d, op.col);
        }
        const bool nul = m.n(0);
        const bool ovf = !nul && (m.o(0) || !ok);
        s.s0 = nul || ovf ? (agg_i128)0 : r;
        m.set(nul, ovf);
        break;
      }
      case AX_CMP: {
        const bool nul = m.n(0) || m.n(1);
        const bool ovf = !nul && (m.o(0) || m.o(1));
        const bool t = !nul && !ovf && agg_cmp_of(op.col, s.s1 < s.s0, s.s1 == s.s0, s.s1 > s.s0);
        s.merge(t ? 1 : 0);
        m.merge(nul, ovf);
        break;
      }
      case AX_IS_NULL:
        s.s0 = m.n(0) ? 1 : 0;
        m.set(false, m.o(0));
        break;
      case AX_AND:
      case AX_OR: {
        bool v, nul, ovf;
        agg_kleene(op.op == AX_OR, s.s1 != 0, m.n(1), m.o(1), s.s0 != 0, m.n(0), m.o(0), &v, &nul, &ovf);
        s.merge(v && !nul && !ovf ? 1 : 0);
        m.merge(nul, ovf);
        break;
      }
      case AX_NOT:
        s.s0 = !m.n(0) && !m.o(0) && s.s0 == 0 ? 1 : 0;
        break;
      case AX_IF: {
        // the condition in slot 2; then below otherwise, or -- col = 1 -- the other way round
        const bool take = !m.n(2) && !m.o(2) && s.s2 != 0;
        const uint32_t at = take != (op.col != 0) ? 1u : 0u;
        const bool co = m.o(2);  // (an overflowed condition: which branch is not known, and that is an overflow)
        const bool nul = !co && m.n(at), ovf = co || m.o(at);
        r = nul || ovf ? (agg_i128)0 : (at ? s.s1 : s.s0);
        s.merge3(r);
        m.merge3(nul, ovf);
        break;
      }
      case AX_COALESCE: {
        const bool b = m.n(1);  // a is NULL: b, with what b carries
        r = b ? s.s0 : s.s1;
        const bool nul = b ? m.n(0) : false, ovf = b ? m.o(0) : m.o(1);
        s.merge(r);
        m.merge(nul, ovf);
        break;
      }
      case AX_SWAP:
        s.swap();
        m.swap();
        break;
      default: break;
    }
  }
  *out = s.s0;
  return m.n(0) ? AGG_ROW_NULL : m.o(0) ? AGG_ROW_OVERFLOW : AGG_ROW_VALUE;
}

// A program of the INT / DEC class on one row.  Row: `bool valid(uint32_t col)`, `agg_i128 load_int(uint32_t col)` (an int64
// column) and `agg_i128 load_dec(uint32_t col)`.  AGG_ROW_NULL: a gating column is NULL, the row contributes nothing;
// AGG_ROW_OVERFLOW: an operation left 128 bits, the row counts and its value is left out; AGG_ROW_VALUE: *out.
// The host's compiler guarantees what is not checked again here: at most four slots in use, operands where an op takes them.
// DIV: the divide is compiled in.  The kernels have an instantiation without it, with the registers they had before there was a
// division, which the host launches for the programs that hold none (agg_ops_hold_division); a division that reaches it all the
// same overflows the row -- never a silent value.
// COND: the interpreter with the conditionals, above -- the third instantiation, with the divide too, launched for the programs
// that hold a conditional op (agg_ops_hold_conditional).  The instantiations without it are, instruction for instruction, what they
// were, and still never hand out a value for such a program: it begins with kAggCondMark, an AX_MOD on the empty, all-zero slots,
// which here is a division the instantiation does not have (DIV = false) or a division by zero (DIV = true) -- `ok` is sticky, the row
// overflows.  (A check of their own in these interpreters was tried in three forms; each cost registers: INTEGRATION.md 6p.)
// CONV: the mixed interpreter, above -- the fourth instantiation, launched for the programs that hold a conversion
// (agg_ops_hold_conversion); the three others are what they were, and a program with conversions overflows the row in each of them
// (agg_program.h: kAggConvMarkCol).
template <bool DIV, bool COND = false, bool CONV = false, typename Row>
AGG_HD int agg_expr_eval_i128_as(const AggExprOp* prog, uint32_t n, const Row& row, agg_i128* out) {
  if constexpr (CONV) return agg_expr_eval_mixed(prog, n, row, false, out);
  if constexpr (COND) return agg_expr_eval_i128_cond<DIV>(prog, n, row, out);
  AggSlots<agg_i128> s = {0, 0, 0, 0};
  bool ok = true;
  for (uint32_t k = 0; k < n; k++) {
    const AggExprOp op = prog[k];
    agg_i128 r = 0;
    switch (op.op) {
      case AX_GATE:
        if (!row.valid(op.col)) return AGG_ROW_NULL;
        break;
      case AX_PUSH_INT: s.push(row.load_int(op.col)); break;
      case AX_PUSH_DEC: s.push(row.load_dec(op.col)); break;
      case AX_PUSH_LIT: s.push(agg_i128_of(op.lo, op.hi)); break;
      case AX_ADD:
        ok &= agg_add_checked(s.s1, s.s0, &r);
        s.merge(r);
        break;
      case AX_SUB:
        ok &= agg_sub_checked(s.s1, s.s0, &r);
        s.merge(r);
        break;
      case AX_RSUB:
        ok &= agg_sub_checked(s.s0, s.s1, &r);
        s.merge(r);
        break;
      case AX_MUL:
        ok &= agg_mul_checked(s.s1, s.s0, &r);
        s.merge(r);
        break;
      case AX_NEG:
        ok &= agg_neg_checked(s.s0, &r);
        s.s0 = r;
        break;
      case AX_SCALE10:
        ok &= agg_mul_checked(s.s0, agg_i128_of(op.lo, op.hi), &r);
        s.s0 = r;
        break;
      case AX_DATE_PART: {
        // the days must be what a Date holds, int32; one outside overflows like an operation that leaves 128 bits.  The calendar
        // works on the 32-bit word alone: the 128-bit slots are not live across it
        const long long d = (long long)s.s0;
        ok &= s.s0 == (agg_i128)(int32_t)d;
        s.s0 = (agg_i128)agg_date_part((int32_t)d, op.col);
        break;
      }
      case AX_DIV:
      case AX_FLOOR_DIV:
      case AX_MOD: {
        if constexpr (!DIV) {
          ok = false;
          s.merge(0);
          break;
        }
        // ONE divide for the three.  The dividend of a Decimal division is first taken times 10^k; where that product leaves 128
        // bits the row overflows, whatever the divide makes of the wrapped value
        agg_i128 a = s.s1;
        if (op.op == AX_DIV && op.col != 0) ok &= agg_mul_checked(a, agg_i128_of(op.lo, op.hi), &a);
        ok &= agg_div_checked(a, s.s0, op.op - AX_DIV, &r);
        s.merge(r);
        break;
      }
      case AX_SWAP: s.swap(); break;
      default: break;
    }
  }
  *out = s.s0;
  return ok ? AGG_ROW_VALUE : AGG_ROW_OVERFLOW;
}

template <typename Row>
AGG_HD int agg_expr_eval_i128(const AggExprOp* prog, uint32_t n, const Row& row, agg_i128* out) {
  return agg_expr_eval_i128_as<true>(prog, n, row, out);
}

// ... of the FLOAT class.  Row: `valid` and `double load_f64(uint32_t col)`.  Every operation is one IEEE double operation.
// (DIV as above; without it a division gives NaN.)
// ... WITH conditionals (agg_expr_eval_i128_cond's counterpart).  No operation on doubles overflows, so a slot has its NULL bit
// alone; a condition is 1.0 / 0.0.  A comparison is IEEE's: with a NaN all are false but !=.
template <bool DIV, typename Row>
AGG_HD int agg_expr_eval_f64_cond(const AggExprOp* prog, uint32_t n, const Row& row, double* out) {
  AggSlots<double> s = {0.0, 0.0, 0.0, 0.0};
  AggSlotBits m = {0, 0};
  // (the mark in front and, in this class, the two ops behind -- agg_program.h: kAggCondMark -- are for the other interpreters)
  const bool marked = agg_cond_marked(prog, n);
  if (marked) n = n >= 1 + kAggCondTailF64 ? n - kAggCondTailF64 : 1;
  for (uint32_t k = marked ? 1 : 0; k < n; k++) {
    const AggExprOp op = prog[k];
    double r = 0.0;
    switch (op.op) {
      case AX_GATE:
        if (!row.valid(op.col)) return AGG_ROW_NULL;
        break;
      case AX_PUSH_F64: {
        const bool v = !op.lo || row.valid(op.col);
        if (v) r = row.load_f64(op.col);
        s.push(r);
        m.push(!v, false);
        break;
      }
      case AX_PUSH_LIT:
        s.push(agg_f64_of_bits(op.lo));
        m.push(false, false);
        break;
      case AX_PUSH_NULL:
        s.push(0.0);
        m.push(true, false);
        break;
      case AX_ADD:
      case AX_SUB:
      case AX_RSUB:
      case AX_MUL:
      case AX_DIV: {
        r = op.op == AX_ADD ? agg_f64_add(s.s1, s.s0) : op.op == AX_SUB ? agg_f64_add(s.s1, -s.s0) : op.op == AX_RSUB ? agg_f64_add(s.s0, -s.s1)
          : op.op == AX_MUL ? agg_f64_mul(s.s1, s.s0) : DIV ? agg_f64_div(s.s1, s.s0) : agg_f64_of_bits(0x7ff8000000000000ull);
        const bool nul = m.n(0) || m.n(1);
        s.merge(nul ? 0.0 : r);
        m.merge(nul, false);
        break;
      }
      case AX_NEG:
        if (!m.n(0)) s.s0 = -s.s0;
        break;
      case AX_ABS:
        if (!m.n(0)) s.s0 = agg_f64_of_bits(agg_bits_of_f64(s.s0) & 0x7fffffffffffffffull);
        break;
      case AX_CMP: {
        const bool nul = m.n(0) || m.n(1);
        const bool t = !nul && agg_cmp_of(op.col, s.s1 < s.s0, s.s1 == s.s0, s.s1 > s.s0);
        s.merge(t ? 1.0 : 0.0);
        m.merge(nul, false);
        break;
      }
      case AX_IS_NULL:
        s.s0 = m.n(0) ? 1.0 : 0.0;
        m.set(false, false);
        break;
      case AX_AND:
      case AX_OR: {
        bool v, nul, ovf;
        agg_kleene(op.op == AX_OR, s.s1 != 0.0, m.n(1), false, s.s0 != 0.0, m.n(0), false, &v, &nul, &ovf);
        s.merge(v && !nul ? 1.0 : 0.0);
        m.merge(nul, false);
        break;
      }
      case AX_NOT:
        s.s0 = !m.n(0) && s.s0 == 0.0 ? 1.0 : 0.0;
        break;
      case AX_IF: {
        const bool take = !m.n(2) && s.s2 != 0.0;
        const uint32_t at = take != (op.col != 0) ? 1u : 0u;
        const bool nul = m.n(at);
        r = nul ? 0.0 : (at ? s.s1 : s.s0);
        s.merge3(r);
        m.merge3(nul, false);
        break;
      }
      case AX_COALESCE: {
        const bool b = m.n(1);
        r = b ? s.s0 : s.s1;
        const bool nul = b && m.n(0);
        s.merge(r);
        m.merge(nul, false);
        break;
      }
      case AX_SWAP:
        s.swap();
        m.swap();
        break;
      default: break;
    }
  }
  *out = s.s0;
  return m.n(0) ? AGG_ROW_NULL : AGG_ROW_VALUE;
}

// (COND as above.  Without it a program with conditionals gives NaN, as a division gives NaN without DIV: the mark is no op of this
// class, but such a program of this class ENDS with `push NaN, add` -- kAggCondTailF64 --, which only these interpreters run.)
// (CONV as above: the mixed interpreter, whose root slot holds the double's bits.  There, and only there, a program of this class
// can overflow a row: a conversion to an integer or a Decimal inside it.)
template <bool DIV, bool COND = false, bool CONV = false, typename Row>
AGG_HD int agg_expr_eval_f64_as(const AggExprOp* prog, uint32_t n, const Row& row, double* out) {
  if constexpr (CONV) {
    agg_i128 v = 0;
    const int rc = agg_expr_eval_mixed(prog, n, row, true, &v);
    *out = agg_f64_of_bits((unsigned long long)v);
    return rc;
  }
  if constexpr (COND) return agg_expr_eval_f64_cond<DIV>(prog, n, row, out);
  AggSlots<double> s = {0.0, 0.0, 0.0, 0.0};
  for (uint32_t k = 0; k < n; k++) {
    const AggExprOp op = prog[k];
    switch (op.op) {
      case AX_GATE:
        if (!row.valid(op.col)) return AGG_ROW_NULL;
        break;
      case AX_PUSH_F64: s.push(row.load_f64(op.col)); break;
      case AX_PUSH_LIT: s.push(agg_f64_of_bits(op.lo)); break;
      case AX_ADD: s.merge(agg_f64_add(s.s1, s.s0)); break;
      case AX_SUB: s.merge(agg_f64_add(s.s1, -s.s0)); break;
      case AX_RSUB: s.merge(agg_f64_add(s.s0, -s.s1)); break;
      case AX_MUL: s.merge(agg_f64_mul(s.s1, s.s0)); break;
      case AX_NEG: s.s0 = -s.s0; break;
      case AX_DIV: s.merge(DIV ? agg_f64_div(s.s1, s.s0) : agg_f64_of_bits(0x7ff8000000000000ull)); break;
      case AX_SWAP: s.swap(); break;
      default: break;
    }
  }
  *out = s.s0;
  return AGG_ROW_VALUE;
}
template <typename Row>
AGG_HD int agg_expr_eval_f64(const AggExprOp* prog, uint32_t n, const Row& row, double* out) {
  return agg_expr_eval_f64_as<true>(prog, n, row, out);
}
#if defined(__clang__)
#pragma clang fp contract(fast)  // (what hipcc builds the rest of the library with)
#endif

// ---- AVG's division: host functions (the device hands over the exact sum and the count) ----

// |w| of a signed 192-bit integer (three little-endian words); returns whether it was negative
inline bool agg_abs192(const unsigned long long* w, unsigned long long* m) {
  const bool neg = (long long)w[2] < 0;
  unsigned long long carry = neg ? 1 : 0;
  for (int k = 0; k < 3; k++) {
    const unsigned long long x = neg ? ~w[k] : w[k];
    m[k] = x + carry;
    carry = carry && m[k] == 0;
  }
  return neg;
}
// m <- m * f (f below 2^64); false when it leaves 192 bits
inline bool agg_mul192_u64(unsigned long long* m, unsigned long long f) {
  unsigned long long carry = 0;
  for (int k = 0; k < 3; k++) {
    const agg_u128 p = (agg_u128)m[k] * f + carry;
    m[k] = (unsigned long long)p;
    carry = (unsigned long long)(p >> 64);
  }
  return carry == 0;
}
// m <- m / d, returns the remainder (d != 0): long division, a 128-by-64 step per word
inline unsigned long long agg_div192_u64(unsigned long long* m, unsigned long long d) {
  unsigned long long rem = 0;
  for (int k = 2; k >= 0; k--) {
    const agg_u128 cur = ((agg_u128)rem << 64) | m[k];
    m[k] = (unsigned long long)(cur / d);
    rem = (unsigned long long)(cur % d);
  }
  return rem;
}
// The average of a Decimal sum `w` (|sum| < 10^38) at scale s over `count` values, at scale min(s + 4, 38): the exact quotient
// rounded half away from zero, as Hive and Spark do.  out: the signed 192-bit result (the caller checks |result| < 10^38).
inline void agg_avg_decimal(const unsigned long long* w, unsigned long long count, uint32_t scale, uint32_t* out_scale, unsigned long long* out) {
  const uint32_t rs = scale + 4 < 38 ? scale + 4 : 38;
  *out_scale = rs;
  unsigned long long m[3];
  const bool neg = agg_abs192(w, m);
  agg_mul192_u64(m, (unsigned long long)agg_pow10(rs - scale));  // (below 10^42: it fits)
  const unsigned long long rem = agg_div192_u64(m, count);
  if (rem >= count - rem) {  // 2 rem >= count: half or more, away from zero
    for (int k = 0; k < 3; k++)
      if (++m[k]) break;
  }
  unsigned long long carry = neg ? 1 : 0;
  for (int k = 0; k < 3; k++) {
    const unsigned long long x = neg ? ~m[k] : m[k];
    out[k] = x + carry;
    carry = carry && out[k] == 0;
  }
}
inline int agg_bits128(agg_u128 v) {
  int n = 0;
  while (v) {
    n++;
    v >>= 1;
  }
  return n;
}
// The double nearest to the exact rational sum / count, ties to even (Python's int / int): sum a signed 128-bit integer
inline double agg_avg_int(agg_i128 sum, unsigned long long count) {
  if (sum == 0) return 0.0;
  const bool neg = sum < 0;
  const agg_u128 n = neg ? (agg_u128)0 - (agg_u128)sum : (agg_u128)sum;
  // a quotient of at least 55 bits, and whether anything is left behind it
  const int want = 56 + agg_bits128(count) - agg_bits128(n), sh = want > 0 ? want : 0;  // (n << sh: at most 120 bits when sh > 0)
  const agg_u128 num = n << sh;
  const agg_u128 q = num / count;
  const bool sticky = num % count != 0;
  const int bq = agg_bits128(q);
  const int drop = bq - 53;  // (bq >= 56: with sh > 0 by the choice of sh, with sh = 0 because bits(n) >= 56 + bits(count))
  unsigned long long mant = (unsigned long long)(q >> drop);
  const agg_u128 rest = q & (((agg_u128)1 << drop) - 1), half = (agg_u128)1 << (drop - 1);
  if (rest > half || (rest == half && (sticky || (mant & 1)))) mant++;
  const double r = __builtin_ldexp((double)mant, drop - sh);
  return neg ? -r : r;
}
