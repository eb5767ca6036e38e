// dictionary_check.cpp -- host-only checks for dictionary output, under AddressSanitizer + UBSan (no GPU, no HIP):
//   1. the name list of orcgpu_reader_set_dictionary_columns (orc_rust_amd/csrc/orcgpu_dictionary_names.inc, the library's own text);
//   2. the counting primitive that keeps a stripe's dictionary alive on the device path: every exported batch of the stripe -- and
//      with it the dictionary array it carries -- holds one reference on the decoded stripe (device_hold.h); the stripe is destroyed
//      exactly once, by whichever release comes last, in every release order.  ONLY the primitive is covered here: the release
//      callbacks that take and drop those references (orcgpu_export.inc, orcgpu_export_device.inc) are HIP text this program cannot
//      compile; they are exercised on the GPU (tests/test_gpu_reader_dictionary.py, tests/test_gpu_device_dictionary.py: batches and
//      tensors read after their siblings and the reader are gone).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../orc_rust_amd/csrc/device_hold.h"
#include "../../orc_rust_amd/csrc/orcgpu_dictionary_names.inc"

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                                    \
    }                                                                \
  } while (0)

static int check(std::vector<const char*> names, std::string* msg = nullptr) {
  static const char* roots[] = {"id", "flag", "mode", "note", "vc", "ch", "bin", ""};
  static const int32_t kinds[] = {4, 7, 7, 7, 16, 17, 8, 7};
  char buf[64];  // (shorter than some messages: they must be cut, not overrun)
  memset(buf, 0x7f, sizeof(buf));
  int rc = orcgpu_host::check_dictionary_names(names.data(), (uint32_t)names.size(), roots, kinds, 8, buf, sizeof(buf));
  if (rc) CHECK(memchr(buf, 0, sizeof(buf)) != nullptr);
  if (msg) *msg = rc ? buf : "";
  return rc;
}

static void names() {
  std::string m;
  CHECK(check({}) == 0);
  CHECK(check({"flag"}) == 0);
  CHECK(check({"flag", "mode", "vc", "ch"}) == 0);
  CHECK(check({"nope"}, &m) == 101 && m.find("nope") != std::string::npos);
  CHECK(check({"flag", "flag"}, &m) == 101 && m.find("flag") != std::string::npos);
  CHECK(check({"mode", "flag", "note", "flag"}, &m) == 101 && m.find("flag") != std::string::npos);
  CHECK(check({"id"}, &m) == 101 && m.find("id") != std::string::npos);
  CHECK(check({"bin"}, &m) == 101 && m.find("bin") != std::string::npos);
  CHECK(check({"flag", nullptr}, &m) == 101);
  CHECK(check({""}) == 0);  // (a root column may have the empty name; Python refuses it before it gets here)
  const std::string longname(1000, 'x');
  CHECK(check({longname.c_str()}, &m) == 101);
  CHECK(orcgpu_host::check_dictionary_names(nullptr, 0, nullptr, nullptr, 0, nullptr, 0) == 0);
  const char* one[] = {"flag"};
  CHECK(orcgpu_host::check_dictionary_names(one, 1, nullptr, nullptr, 0, nullptr, 0) == 101);
}

struct Stripe {
  int* destroyed;
  std::vector<int> dictionary;  // what the batches share
};
static void destroy_stripe(void* p) {
  Stripe* s = static_cast<Stripe*>(p);
  (*s->destroyed)++;
  delete s;
}

static void release_orders() {
  const int n_batches = 4;
  std::vector<int> order(n_batches + 1);  // n_batches exports and the owner (index n_batches)
  for (int k = 0; k <= n_batches; k++) order[k] = k;
  int runs = 0;
  do {
    int destroyed = 0;
    Stripe* s = new Stripe{&destroyed, std::vector<int>(100, 7)};
    orcgpu_hold::Hold* h = orcgpu_hold::hold_new(s, destroy_stripe, nullptr);
    for (int k = 0; k < n_batches; k++) orcgpu_hold::hold_acquire(h);
    for (int k = 0; k <= n_batches; k++) {
      CHECK(destroyed == 0);
      if (k) CHECK(s->dictionary[99] == 7);  // still readable while anything refers to it (ASan: no use after free)
      if (order[k] == n_batches) orcgpu_hold::hold_owner_done(h, false);
      else orcgpu_hold::hold_release(h);
    }
    CHECK(destroyed == 1);
    runs++;
  } while (std::next_permutation(order.begin(), order.end()));
  CHECK(runs == 120);
}

int main() {
  names();
  release_orders();
  if (failures) return 1;
  printf("dictionary_check ok\n");
  return 0;
}
