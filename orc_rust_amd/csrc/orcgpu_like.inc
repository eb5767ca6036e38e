// orcgpu_like.inc -- a SQL LIKE pattern taken apart, host only: shared by the row filter's plan compiler (orcgpu_filter_plan.inc)
// and the row-group pruning (orcgpu_predicate.inc).  The semantics are those of include/orcgpu.h (ORCGPU_PRED_LIKE).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace orcgpu_host {

enum { LIKE_EL_BYTE = 0, LIKE_EL_ONE = 1 /* _ */, LIKE_EL_ANY = 2 /* % */ };

struct LikePattern {
  std::vector<uint8_t> bytes;  // per element: the literal byte (0 for a wildcard)
  std::vector<uint8_t> kinds;  // per element: LIKE_EL_*
  bool wildcard_free() const {
    for (uint8_t k : kinds)
      if (k != LIKE_EL_BYTE) return false;
    return true;
  }
  // the literal bytes in front of the first wildcard
  std::string prefix() const {
    std::string p;
    for (size_t k = 0; k < kinds.size() && kinds[k] == LIKE_EL_BYTE; k++) p.push_back((char)bytes[k]);
    return p;
  }
};

// The pattern's elements with the escape byte (0: none) applied: it makes the byte behind it a literal, whatever that byte is.
// false: the pattern ends in the escape byte.
inline bool like_unescape(const char* s, size_t n, int escape, LikePattern& out) {
  out.bytes.clear();
  out.kinds.clear();
  for (size_t k = 0; k < n; k++) {
    const uint8_t b = (uint8_t)s[k];
    if (escape && b == (uint8_t)escape) {
      if (k + 1 == n) return false;
      out.bytes.push_back((uint8_t)s[++k]);
      out.kinds.push_back(LIKE_EL_BYTE);
    } else if (b == '%' || b == '_') {
      out.bytes.push_back(0);
      out.kinds.push_back(b == '%' ? LIKE_EL_ANY : LIKE_EL_ONE);
    } else {
      out.bytes.push_back(b);
      out.kinds.push_back(LIKE_EL_BYTE);
    }
  }
  return true;
}

// succ(p): the smallest string above every string that begins with p -- p with its last byte that is not 0xFF incremented and
// everything behind it cut off.  false: p is all 0xFF (or empty), nothing is above.
inline bool like_prefix_succ(const std::string& p, std::string& out) {
  size_t n = p.size();
  while (n && (uint8_t)p[n - 1] == 0xFF) n--;
  if (!n) return false;
  out.assign(p, 0, n);
  out[n - 1] = (char)((uint8_t)out[n - 1] + 1);
  return true;
}

}  // namespace orcgpu_host
