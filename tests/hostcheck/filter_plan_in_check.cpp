// filter_plan_in_check.cpp -- IN lists through the row filter's plan compiler (orc_rust_amd/csrc/orcgpu_filter_plan.inc and
// orcgpu_in.inc, the very text liborcgpu.so is built from) under AddressSanitizer + UBSan, on the CPU (TEST INFRASTRUCTURE).
// The program judges nothing but the bounds of what the compiler wrote: it prints what became of every list and
// tests/test_filter_plan_in_sanitized.py checks the lines -- it probes every table by the rule written down in
// device/filter_program.h.
//
// argv[1]: a file of cases, one per line:  <name> <column> <leaf | not | nested> <literal> ...
//   literal: <value_type>:<1 when NULL>:<i>:<the double's bits in hex>:<s in hex, = for the empty string, or - for none>
//   (every string in a heap block of exactly its size: a read past its end is a report)
// Output, per case:
//   in <name> <status> <1 when the message names the column> <instructions> <op> <cmp> <i> <lo> <bits of f> <lit_off> <lit_len> <hex or ->
//     of the FIRST instruction; hex: the table of a FOP_IN with one, the literal of a string comparison.
// ... and for the node lists built in here:
//   bad <name> <status> <1 when the message names the column>
//   planes <op, i and cmp of every instruction of a program with two IN leaves and a LIKE leaf>
//   leaves like <instruction indices of that program's LIKE leaves with a plane> in <... of its IN leaves with a table>
//   depth <status of an IN leaf at the deepest level allowed> <status one level deeper>
// Exit code 0 whenever the compiler RETURNED; a sanitizer report aborts with its own exit code.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/orcgpu.h"
#include "../../orc_rust_amd/csrc/orcgpu_filter_plan.inc"

using namespace orcgpu_host;

static const char* kNames[] = {"i8", "i16", "i32", "i64", "date", "f32", "f64", "b", "s", "bin", "vc", "ch", "dec", "ts", "ts9", "st"};
static const int32_t kKinds[] = {ORCGPU_T_BYTE, ORCGPU_T_SHORT, ORCGPU_T_INT, ORCGPU_T_LONG, ORCGPU_T_DATE, ORCGPU_T_FLOAT, ORCGPU_T_DOUBLE, ORCGPU_T_BOOLEAN,
                                 ORCGPU_T_STRING, ORCGPU_T_BINARY, ORCGPU_T_VARCHAR, ORCGPU_T_CHAR, ORCGPU_T_DECIMAL, ORCGPU_T_TIMESTAMP, ORCGPU_T_TIMESTAMP_INSTANT,
                                 ORCGPU_T_STRUCT};
// a Decimal(.., 2) column, a Timestamp decoded to microseconds and one decoded to Decimal128(38, 9)
static const int32_t kParams[] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 4, 0};
constexpr uint32_t kColumns = 15;  // (without the Struct)

static std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s(2 * n, '0');
  for (size_t k = 0; k < n; k++) {
    s[2 * k] = d[p[k] >> 4];
    s[2 * k + 1] = d[p[k] & 15];
  }
  return s;
}
static int nibble(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

struct Holder {  // keeps the strings of a node list alive, each in its own heap block
  std::vector<std::unique_ptr<char[]>> blocks;
  const char* put(const std::string& h) {
    blocks.emplace_back(new char[h.size() / 2 ? h.size() / 2 : 1]);
    for (size_t k = 0; k + 1 < h.size(); k += 2) blocks.back()[k / 2] = (char)(nibble(h[k]) << 4 | nibble(h[k + 1]));
    return blocks.back().get();
  }
};

static orcgpu_predicate_node literal_node(const std::string& tok, Holder& hold) {
  std::vector<std::string> f;
  std::stringstream ss(tok);
  for (std::string part; std::getline(ss, part, ':');) f.push_back(part);
  if (f.size() != 5) abort();
  orcgpu_predicate_node n{};
  n.op = ORCGPU_PRED_LITERAL;
  n.value_type = atoi(f[0].c_str());
  n.value_is_null = atoi(f[1].c_str());
  n.i = strtoll(f[2].c_str(), nullptr, 10);
  const unsigned long long bits = strtoull(f[3].c_str(), nullptr, 16);
  memcpy(&n.f, &bits, 8);
  if (f[4] == "=") n.s = hold.put("");  // the empty string, with bytes to point at
  else if (f[4] != "-") {
    n.s = hold.put(f[4]);
    n.s_len = f[4].size() / 2;
  }
  return n;
}
static orcgpu_predicate_node in_node(const char* col, uint32_t k) {
  orcgpu_predicate_node n{};
  n.op = ORCGPU_PRED_IN;
  n.column = col;
  n.n_children = k;
  return n;
}
static orcgpu_predicate_node int_literal(long long v) {
  orcgpu_predicate_node n{};
  n.op = ORCGPU_PRED_LITERAL;
  n.value_type = ORCGPU_PV_INT64;
  n.i = v;
  return n;
}

static void report(const char* tag, const std::string& name, const std::string& col, int rc, const FilterPlan& plan, bool first) {
  const int named = strstr(plan.err, ("'" + col + "'").c_str()) ? 1 : 0;
  if (rc && !plan.err[0]) abort();
  if (!first || rc || plan.prog.empty()) {
    printf("%s %s %d %d\n", tag, name.c_str(), rc, named);
    return;
  }
  const FilterInsn& in = plan.prog[0];
  std::string payload = "-";
  if ((in.op == FOP_IN && !(in.cmp & IN_NO_TABLE)) || in.op == FOP_CMP_STRING) {
    if (in.lit_off + in.lit_len > plan.lits.size()) abort();
    if (in.op == FOP_IN && ((in.lit_off & 7) || (in.lit_len & 7) || in.lit_len < kInHeaderBytes)) abort();
    payload = in.lit_len ? hex(plan.lits.data() + in.lit_off, in.lit_len) : "=";
  }
  unsigned long long bits;
  memcpy(&bits, &in.f, 8);
  printf("%s %s %d %d %zu %u %u %lld %llu %llx %llu %u %s\n", tag, name.c_str(), rc, named, plan.prog.size(), in.op, in.cmp, in.i, in.lo, bits, in.lit_off, in.lit_len,
         payload.c_str());
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::ifstream cases(argv[1]);
  for (std::string line; std::getline(cases, line);) {
    std::stringstream ss(line);
    std::string name, col, wrap, tok;
    ss >> name >> col >> wrap;
    Holder hold;
    std::vector<orcgpu_predicate_node> nodes;
    if (wrap == "not") {
      orcgpu_predicate_node n{};
      n.op = ORCGPU_PRED_NOT;
      n.n_children = 1;
      nodes.push_back(n);
    }
    const size_t leaf = nodes.size();
    nodes.push_back(in_node(col.c_str(), 0));
    while (ss >> tok) nodes.push_back(literal_node(tok, hold));
    nodes[leaf].n_children = (uint32_t)(nodes.size() - leaf - 1);
    // (the node list itself in a heap block of exactly its size)
    std::unique_ptr<orcgpu_predicate_node[]> heap(new orcgpu_predicate_node[nodes.size()]);
    for (size_t k = 0; k < nodes.size(); k++) heap[k] = nodes[k];
    FilterPlan plan;
    const int rc = filter_compile(heap.get(), (uint32_t)nodes.size(), kNames, kKinds, wrap == "nested" ? kColumns + 1 : kColumns, plan, kParams);
    if (!rc && plan.depth != (wrap == "not" ? 2u : 1u)) abort();
    report("in", name, wrap == "nested" ? "st" : col, rc, plan, true);
  }
  // ---- malformed node lists ----
  auto bad = [&](const char* name, const char* col, std::vector<orcgpu_predicate_node> nodes) {
    std::unique_ptr<orcgpu_predicate_node[]> heap(new orcgpu_predicate_node[nodes.size() ? nodes.size() : 1]);
    for (size_t k = 0; k < nodes.size(); k++) heap[k] = nodes[k];
    FilterPlan plan;
    const int rc = filter_compile(heap.get(), (uint32_t)nodes.size(), kNames, kKinds, kColumns, plan, kParams);
    report("bad", name, col, rc, plan, false);
  };
  orcgpu_predicate_node eq{};
  eq.op = ORCGPU_PRED_EQ;
  eq.column = "i64";
  eq.value_type = ORCGPU_PV_INT64;
  orcgpu_predicate_node and2{}, or2{}, not1{};
  and2.op = ORCGPU_PRED_AND;
  or2.op = ORCGPU_PRED_OR;
  and2.n_children = or2.n_children = 2;
  not1.op = ORCGPU_PRED_NOT;
  not1.n_children = 1;
  orcgpu_predicate_node with_kid = int_literal(3);
  with_kid.n_children = 1;
  orcgpu_predicate_node named = int_literal(3);
  named.column = "i64";
  bad("literal_alone", "i64", {int_literal(1)});
  bad("literal_under_and", "i64", {and2, eq, int_literal(1)});
  bad("literal_under_not", "i64", {not1, int_literal(1)});
  bad("literal_behind_the_list", "i64", {and2, in_node("i64", 1), int_literal(1), int_literal(2)});
  bad("child_is_a_comparison", "i64", {in_node("i64", 2), int_literal(1), eq});
  bad("child_is_an_in", "i64", {in_node("i64", 2), int_literal(1), in_node("i64", 0)});
  bad("literal_with_children", "i64", {in_node("i64", 2), int_literal(1), with_kid, int_literal(2)});
  bad("list_ends_early", "i64", {in_node("i64", 3), int_literal(1), int_literal(2)});
  bad("list_ends_early_in_a_tree", "i64", {or2, eq, in_node("i64", 2), int_literal(1)});
  bad("nodes_behind_the_root", "i64", {in_node("i64", 1), int_literal(1), int_literal(2)});
  bad("no_column_name", "i64", {in_node(nullptr, 1), int_literal(1)});
  bad("no_such_column", "nope", {in_node("nope", 1), int_literal(1)});
  bad("literal_with_a_column_is_fine", "i64", {in_node("i64", 2), named, int_literal(4)});
  bad("op_11_is_unknown", "i64", {[] {
        orcgpu_predicate_node n{};
        n.op = 11;
        n.column = "i64";
        return n;
      }()});
  {
    // two IN leaves and a LIKE leaf: the planes are numbered together, in the order of the leaves; a one-key list, a Boolean
    // list and an empty list take none
    orcgpu_predicate_node root{};
    root.op = ORCGPU_PRED_OR;
    root.n_children = 6;
    orcgpu_predicate_node like{};
    like.op = ORCGPU_PRED_LIKE;
    like.column = "s";
    like.value_type = ORCGPU_PV_UTF8;
    like.s = "a%";
    like.s_len = 2;
    orcgpu_predicate_node t{}, f{}, str{};
    t.op = f.op = str.op = ORCGPU_PRED_LITERAL;
    t.value_type = f.value_type = ORCGPU_PV_BOOLEAN;
    t.i = 1;
    str.value_type = ORCGPU_PV_UTF8;
    str.s = "xy";
    str.s_len = 2;
    orcgpu_predicate_node str2 = str;
    str2.s = "z";
    str2.s_len = 1;
    std::vector<orcgpu_predicate_node> nodes = {root, in_node("i64", 2), int_literal(1), int_literal(2), in_node("i32", 1), int_literal(5), like,
                                                in_node("b", 2), t, f, in_node("vc", 2), str, str2, in_node("i8", 0)};
    FilterPlan plan;
    if (filter_compile(nodes.data(), (uint32_t)nodes.size(), kNames, kKinds, kColumns, plan, kParams)) abort();
    printf("planes");
    for (const FilterInsn& in : plan.prog) printf(" %u:%lld:%u", in.op, in.i, in.cmp);
    printf("\nleaves like");
    for (uint32_t k : plan.like_leaves) printf(" %u", k);
    printf(" in");
    for (uint32_t k : plan.in_leaves) printf(" %u", k);
    printf("\n");
    for (const FilterInsn& in : plan.prog)
      if (in.op == FOP_IN && !(in.cmp & IN_NO_TABLE) && ((in.lit_off & 7) || in.lit_off + in.lit_len > plan.lits.size())) abort();
  }
  {
    // the list counts as the leaf alone: 63 NOTs above an IN of three are 64 levels, 64 NOTs are one too many
    int rcs[2];
    for (int extra = 0; extra < 2; extra++) {
      std::vector<orcgpu_predicate_node> nodes((size_t)ORCGPU_FILTER_MAX_DEPTH - 1 + extra, not1);
      nodes.push_back(in_node("i64", 3));
      for (int k = 0; k < 3; k++) nodes.push_back(int_literal(k));
      FilterPlan plan;
      rcs[extra] = filter_compile(nodes.data(), (uint32_t)nodes.size(), kNames, kKinds, kColumns, plan, kParams);
    }
    printf("depth %d %d\n", rcs[0], rcs[1]);
  }
  return 0;
}
