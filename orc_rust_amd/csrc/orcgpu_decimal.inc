// orcgpu_decimal.inc -- exact decimal arithmetic for predicates, host only and free of HIP: a Decimal128 literal
// (ORCGPU_PV_DECIMAL128) off its 16 bytes, floor division by a power of ten, the order of two (unscaled, scale) pairs as
// rationals, the decimal strings of ORC's DecimalStatistics, and the "might match" rules on them.  Used by the row filter's plan
// compiler (orcgpu_filter_plan.inc) and by the row-group pruning (orcgpu_predicate.inc);
// tests/hostcheck/filter_plan_typed_check.cpp compiles this very text under AddressSanitizer + UBSan.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

namespace orcgpu_host {

typedef __int128 i128;
constexpr int kDecMaxDigits = 38;  // Decimal128: |unscaled| < 10^38 < 2^127

inline i128 dec_pow10(int e) {  // 0 <= e <= 38
  i128 p = 1;
  for (int k = 0; k < e; k++) p *= 10;
  return p;
}
inline i128 dec_i128_max() { return (i128)(~(unsigned __int128)0 >> 1); }
inline i128 dec_i128_min() { return -dec_i128_max() - 1; }

// The literal of a ORCGPU_PV_DECIMAL128 node: 16 bytes little-endian two's complement with |value| < 10^38, scale 0 .. 38
inline bool dec_literal(const char* s, uint64_t s_len, int64_t scale, i128& unscaled) {
  if (!s || s_len != 16 || scale < 0 || scale > kDecMaxDigits) return false;
  unsigned __int128 u = 0;
  for (int k = 15; k >= 0; k--) u = (u << 8) | (uint8_t)s[k];
  unscaled = (i128)u;
  const i128 lim = dec_pow10(kDecMaxDigits);
  return unscaled > -lim && unscaled < lim;
}

// v * 10^e (e >= 0); false when the product leaves int128
inline bool dec_scale_up(i128 v, int e, i128& out) {
  for (int k = 0; k < e; k++)
    if (__builtin_mul_overflow(v, (i128)10, &v)) return false;
  out = v;
  return true;
}

// q = floor(v / 10^e), r = v - q * 10^e >= 0 (e >= 0; a power of ten beyond int128 is above every |v|)
inline void dec_floor_div(i128 v, int e, i128& q, bool& exact) {
  if (e > kDecMaxDigits) {
    q = v < 0 ? -1 : 0;
    exact = v == 0;
    return;
  }
  const i128 p = dec_pow10(e);
  q = v / p;
  i128 r = v % p;
  if (r < 0) {  // (C++ truncates toward zero)
    q -= 1;
    r += p;
  }
  exact = r == 0;
}

// a * 10^-sa against b * 10^-sb: -1, 0, +1
inline int dec_cmp(i128 a, int sa, i128 b, int sb) {
  if (sa == sb) return a < b ? -1 : (a > b ? 1 : 0);
  if (sa > sb) return -dec_cmp(b, sb, a, sa);
  // a * 10^d against b with d = sb - sa > 0: a against floor(b / 10^d), a tie broken by the remainder
  i128 q;
  bool exact;
  dec_floor_div(b, sb - sa, q, exact);
  if (a != q) return a < q ? -1 : 1;
  return exact ? 0 : -1;
}

// A decimal as Apache ORC prints it into DecimalStatistics (Decimal::toString / HiveDecimal): sign, digits, optional fraction,
// optional exponent.  -> unscaled * 10^-scale with |unscaled| < 10^38 and scale >= 0; false on anything else
inline bool dec_parse(const std::string& s, i128& unscaled, int& scale) {
  size_t at = 0;
  bool neg = false;
  if (at < s.size() && (s[at] == '+' || s[at] == '-')) neg = s[at++] == '-';
  i128 v = 0;
  int digits = 0, frac = 0, significant = 0;
  bool in_frac = false;
  for (; at < s.size(); at++) {
    const char c = s[at];
    if (c == '.' && !in_frac) {
      in_frac = true;
      continue;
    }
    if (c < '0' || c > '9') break;
    if (significant || c != '0') significant++;
    if (significant > kDecMaxDigits) return false;
    v = v * 10 + (c - '0');
    digits++;
    if (in_frac) frac++;
  }
  if (!digits) return false;
  long long exp10 = 0;
  if (at < s.size() && (s[at] == 'e' || s[at] == 'E')) {
    at++;
    bool eneg = false;
    if (at < s.size() && (s[at] == '+' || s[at] == '-')) eneg = s[at++] == '-';
    int edigits = 0;
    for (; at < s.size() && s[at] >= '0' && s[at] <= '9'; at++, edigits++) {
      exp10 = exp10 * 10 + (s[at] - '0');
      if (exp10 > 1000) return false;
    }
    if (!edigits) return false;
    if (eneg) exp10 = -exp10;
  }
  if (at != s.size()) return false;
  long long sc = (long long)frac - exp10;
  if (sc < 0) {  // "1E+2": an integer with trailing zeros
    if (v != 0 && significant - sc > kDecMaxDigits) return false;
    if (v != 0 && !dec_scale_up(v, (int)-sc, v)) return false;
    sc = 0;
  }
  if (v == 0) sc = 0;
  unscaled = neg ? -v : v;
  scale = (int)sc;
  return true;
}

// row_group_filter.rs' "might match" rules (cmp_int's) over a group's [min, max], in exact rational order
inline bool dec_might_match(i128 mn, int mn_scale, i128 mx, int mx_scale, int op, i128 v, int v_scale) {
  const int lo = dec_cmp(mn, mn_scale, v, v_scale), hi = dec_cmp(mx, mx_scale, v, v_scale);
  switch (op) {
    case ORCGPU_PRED_EQ: return lo <= 0 && hi >= 0;
    case ORCGPU_PRED_NE: return !(lo == 0 && hi == 0);
    case ORCGPU_PRED_LT: return lo < 0;
    case ORCGPU_PRED_LE: return lo <= 0;
    case ORCGPU_PRED_GT: return hi > 0;
    default: return hi >= 0;
  }
}

// DecimalStatistics' minimum / maximum strings against a Decimal128 literal.  false: a string does not parse (the evaluation
// fails and the stripe is read whole); else *match says whether the group might hold a matching row
inline bool dec_stats_match(const std::string& smin, const std::string& smax, int op, i128 v, int v_scale, bool* match) {
  i128 mn, mx;
  int mn_scale, mx_scale;
  if (!dec_parse(smin, mn, mn_scale) || !dec_parse(smax, mx, mx_scale)) return false;
  *match = dec_might_match(mn, mn_scale, mx, mx_scale, op, v, v_scale);
  return true;
}

}  // namespace orcgpu_host
