// orcgpu_dictionary_names.inc -- the name list of orcgpu_reader_set_dictionary_columns against a file's root columns.  Host only
// and free of HIP (tests/hostcheck/dictionary_check.cpp compiles this very text under AddressSanitizer + UBSan).
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace orcgpu_host {

// names[n] against the root columns (roots[n_roots], their ORC kinds).  Every name must be a root column of kind STRING (7),
// VARCHAR (16) or CHAR (17) and appear once.  0, or ORCGPU_INVALID_ARGUMENT (101) with a message that names the offender.
inline int check_dictionary_names(const char* const* names, uint32_t n, const char* const* roots, const int32_t* kinds, uint32_t n_roots, char* msg,
                                  size_t msg_cap) {
  auto fail = [&](const char* fmt, const char* a, int b) {
    if (msg && msg_cap) snprintf(msg, msg_cap, fmt, a, b);
    return 101;
  };
  for (uint32_t i = 0; i < n; i++) {
    if (!names[i]) return fail("dictionary columns: name %s%d is NULL", "", (int)i);
    for (uint32_t k = 0; k < i; k++)
      if (!strcmp(names[k], names[i])) return fail("dictionary columns: '%s' is listed twice (at %d)", names[i], (int)i);
    uint32_t at = n_roots;
    for (uint32_t k = 0; k < n_roots && at == n_roots; k++)
      if (roots[k] && !strcmp(roots[k], names[i])) at = k;
    if (at == n_roots) return fail("dictionary columns: the file has no root column '%s' (name %d)", names[i], (int)i);
    if (kinds[at] != 7 && kinds[at] != 16 && kinds[at] != 17)
      return fail("dictionary columns: column '%s' is of ORC type kind %d, not STRING / VARCHAR / CHAR", names[i], kinds[at]);
  }
  return 0;
}

}  // namespace orcgpu_host
