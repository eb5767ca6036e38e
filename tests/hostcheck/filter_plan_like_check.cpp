// filter_plan_like_check.cpp -- LIKE patterns through the row filter's plan compiler (orc_rust_amd/csrc/orcgpu_filter_plan.inc and
// orcgpu_like.inc, the very text liborcgpu.so is built from) under AddressSanitizer + UBSan, on the CPU (TEST INFRASTRUCTURE).
// The program judges nothing but the bounds of what the compiler wrote: it prints what became of every pattern and
// tests/test_filter_plan_like_sanitized.py compares the lines with tests/like_model.py.
//
//   pat <pattern in hex, or -> <escape> <status> <class> <anchors and parts, or ->
//     class: eq (FOP_CMP_STRING EQ on the unescaped bytes), unknown (FOP_UNKNOWN), all / prefix / suffix / contains / general
//     (FOP_LIKE with that shape), - (refused).  Parts: S or - (anchored at the start), the parts' elements in hex with __ for a
//     `_`, joined by |, then E or -; for eq the unescaped bytes.
//   bad <name> <status> <1 when the message names the column>
// Exit code 0 whenever the compiler RETURNED; a sanitizer report aborts with its own exit code.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../include/orcgpu.h"
#include "../../orc_rust_amd/csrc/orcgpu_filter_plan.inc"

using namespace orcgpu_host;

static const char* kNames[] = {"i", "s", "bin", "vc", "ch"};
static const int32_t kKinds[] = {ORCGPU_T_LONG, ORCGPU_T_STRING, ORCGPU_T_BINARY, ORCGPU_T_VARCHAR, ORCGPU_T_CHAR};

static orcgpu_predicate_node like_node(const char* col, const char* s, uint64_t s_len, int64_t escape, int vt = ORCGPU_PV_UTF8, int is_null = 0) {
  orcgpu_predicate_node n{};
  n.op = ORCGPU_PRED_LIKE;
  n.column = col;
  n.value_type = vt;
  n.value_is_null = is_null;
  n.i = escape;
  n.s = s;
  n.s_len = s_len;
  return n;
}
static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (size_t k = 0; k < n; k++) {
    s.push_back(d[p[k] >> 4]);
    s.push_back(d[p[k] & 15]);
  }
  return s;
}
static uint32_t word(const FilterPlan& plan, uint64_t at) {
  if (at + 4 > plan.lits.size()) abort();
  return plan.lits[at] | plan.lits[at + 1] << 8 | plan.lits[at + 2] << 16 | (uint32_t)plan.lits[at + 3] << 24;
}

static void pat(const std::string& p, int escape, const char* col = "s") {
  // (the pattern in a heap block of exactly its size: a read past its end is a report)
  std::vector<char> heap(p.begin(), p.end());
  const orcgpu_predicate_node n = like_node(col, heap.empty() ? "" : heap.data(), heap.size(), escape);
  FilterPlan plan;
  const int rc = filter_compile(&n, 1, kNames, kKinds, 5, plan);
  std::string cls = "-", parts = "-";
  if (!rc) {
    if (plan.prog.size() != 1 || plan.depth != 1) abort();
    const FilterInsn& in = plan.prog[0];
    if (in.op == FOP_CMP_STRING) {
      if (in.cmp != ORCGPU_PRED_EQ || in.lit_off + in.lit_len > plan.lits.size()) abort();
      cls = "eq";
      parts = "=" + hex(plan.lits.data() + in.lit_off, in.lit_len);
    } else if (in.op == FOP_LIKE && in.cmp == LIKE_ALL) {
      if (in.lit_len) abort();
      cls = "all";
    } else if (in.op == FOP_LIKE) {
      static const char* names[] = {"all", "prefix", "suffix", "contains", "general"};
      if (in.cmp > LIKE_GENERAL || in.i != 0 || (in.lit_off & 3) || in.lit_off + in.lit_len > plan.lits.size() || in.lit_len > kLikeBlobMax) abort();
      const uint32_t shape = word(plan, in.lit_off), flags = word(plan, in.lit_off + 4), np = word(plan, in.lit_off + 8), ne = word(plan, in.lit_off + 12);
      if (shape != in.cmp || flags > 3 || !np || np > kLikeMaxParts || !ne || ne > kLikeMaxBytes || in.lit_len != (kLikeHeaderWords + 2 * np) * 4 + 2 * ne) abort();
      const uint8_t* bytes = plan.lits.data() + in.lit_off + (kLikeHeaderWords + 2 * np) * 4;
      const uint8_t* ones = bytes + ne;
      cls = names[shape];
      parts = flags & LIKE_ANCHOR_START ? "S" : "-";
      uint32_t next = 0;
      for (uint32_t k = 0; k < np; k++) {
        const uint32_t first = word(plan, in.lit_off + 16 + 8 * k), len = word(plan, in.lit_off + 20 + 8 * k);
        if (first != next || !len || first + len > ne) abort();  // the parts tile the element arrays
        next = first + len;
        if (k) parts += "|";
        for (uint32_t e = first; e < first + len; e++) {
          if (ones[e] > 1 || (ones[e] && bytes[e])) abort();
          parts += ones[e] ? "__" : hex(bytes + e, 1);
        }
      }
      if (next != ne) abort();
      parts += flags & LIKE_ANCHOR_END ? "E" : "-";
    } else if (in.op == FOP_UNKNOWN) cls = "unknown";
    else abort();
  } else if (!plan.err[0]) abort();
  printf("pat %s %d %d %s %s\n", p.empty() ? "-" : hex(reinterpret_cast<const uint8_t*>(p.data()), p.size()).c_str(), escape, rc, cls.c_str(), parts.c_str());
}
static void bad(const char* name, const char* col, const orcgpu_predicate_node& n, uint32_t n_columns = 5) {
  FilterPlan plan;
  const int rc = filter_compile(&n, 1, kNames, kKinds, n_columns, plan);
  printf("bad %s %d %d %zu %d\n", name, rc, strstr(plan.err, (std::string("'") + col + "'").c_str()) ? 1 : 0, plan.prog.size(),
         plan.prog.empty() ? -1 : (int)plan.prog[0].op);
}

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1;
  const int n_random = argc > 2 ? atoi(argv[2]) : 3000;
  // ---- the corner patterns of the tests, under a backslash, another escape and none ----
  const std::string corner[] = {"", "%", "%%", "_", "__", "%_%", "a%", "%a", "%aab", "ab%ba", "%a%a%", "h_llo", "h_", "_\xc3\xa9", "a\\%b", "a\\_b",
                                "a\\\\b", "%\n%", "a%b%a", "%a%b%a%b%a%", "%aab%", "aab%", "_\xf0\x9f\x98\x80%", "%c_abc", "a!%b", "a#_b", "%!_%",
                                "a!\\b", "%%a%%", "a%%", "\\%", "\\_", "%\\%%", "\xff\xfe%", std::string("a\0b%", 4), "a\\"};
  for (const std::string& p : corner)
    for (int escape : {(int)'\\', (int)'!', 0}) pat(p, escape);
  pat("a%", '\\', "vc");
  pat("%a", '\\', "ch");
  // ---- the limits ----
  pat(std::string(1024, 'a'), '\\');
  pat(std::string(1025, 'a'), '\\');
  pat(std::string(1023, 'a') + "%", '\\');
  pat(std::string(1024, 'a') + "%", '\\');
  pat(std::string(1024, '%'), '\\');
  pat(std::string(1025, '_'), '\\');
  {
    std::string twice, more, parts64 = "a", parts65, huge(5000, 'a');
    for (int k = 0; k < 1024; k++) twice += "\\%";  // 2048 bytes, 1024 after unescaping
    more = twice + "x";
    for (int k = 1; k < 64; k++) parts64 += "%b";
    parts65 = parts64 + "%c";
    for (const std::string& p : {twice, more, parts64, parts65, "%" + parts64 + "%", "%" + parts65 + "%", huge}) pat(p, '\\');
  }
  // ---- refusals ----
  bad("trailing_escape", "s", like_node("s", "ab!", 3, '!'));
  bad("escape_200", "s", like_node("s", "a%", 2, 200));
  bad("escape_negative", "s", like_node("s", "a%", 2, -1));
  bad("escape_128", "s", like_node("s", "a%", 2, 128));
  bad("binary_column", "bin", like_node("bin", "a%", 2, 0));
  bad("int_column", "i", like_node("i", "a%", 2, 0));
  bad("int64_literal", "s", like_node("s", "a%", 2, 0, ORCGPU_PV_INT64));
  bad("null_pattern", "s", like_node("s", nullptr, 0, 0, ORCGPU_PV_UTF8, 1));
  bad("null_pattern_on_int", "i", like_node("i", nullptr, 0, 0, ORCGPU_PV_UTF8, 1));
  bad("length_without_bytes", "s", like_node("s", nullptr, 3, 0));
  bad("no_such_column", "nope", like_node("nope", "a%", 2, 0));
  bad("no_column_name", "s", like_node(nullptr, "a%", 2, 0));
  {
    orcgpu_predicate_node with_child = like_node("s", "a%", 2, 0);
    with_child.n_children = 0;
    std::vector<orcgpu_predicate_node> under_not(3);
    under_not[0].op = ORCGPU_PRED_NOT;
    under_not[0].n_children = 1;
    under_not[1].op = ORCGPU_PRED_AND;
    under_not[1].n_children = 1;
    under_not[2] = with_child;
    FilterPlan plan;
    const int rc = filter_compile(under_not.data(), 3, kNames, kKinds, 5, plan);
    printf("tree not_and_like %d %zu %d\n", rc, plan.prog.size(), rc ? -1 : (int)plan.prog[0].op);
    // two LIKE leaves get two mask planes, a keep-all leaf between them none
    std::vector<orcgpu_predicate_node> three(4);
    three[0].op = ORCGPU_PRED_OR;
    three[0].n_children = 3;
    three[1] = like_node("s", "a%", 2, 0);
    three[2] = like_node("vc", "%", 1, 0);
    three[3] = like_node("ch", "%b_", 3, 0);
    const int rc3 = filter_compile(three.data(), 4, kNames, kKinds, 5, plan);
    if (rc3 || plan.prog.size() != 5) abort();
    printf("planes %lld %u %lld\n", plan.prog[0].i, plan.prog[1].cmp, plan.prog[3].i);
  }
  // ---- seeded random patterns over an alphabet that is mostly syntax ----
  std::mt19937 rng(seed);
  const char alphabet[] = {'%', '_', '\\', '!', 'a', 'b', (char)0xc3, (char)0xa9, '\n', (char)0xff, 0};
  for (int k = 0; k < n_random; k++) {
    const size_t n = rng() % (k % 50 == 0 ? 1100 : 12);
    std::string p;
    for (size_t x = 0; x < n; x++) p.push_back(alphabet[rng() % sizeof(alphabet)]);
    static const int escapes[3] = {'\\', '!', 0};
    pat(p, escapes[rng() % 3]);
  }
  return 0;
}
