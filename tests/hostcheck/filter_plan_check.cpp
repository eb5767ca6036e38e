// filter_plan_check.cpp -- the row filter's plan compiler (orc_rust_amd/csrc/orcgpu_filter_plan.inc, the very text liborcgpu.so is
// built from) under AddressSanitizer + UBSan, on the CPU (TEST INFRASTRUCTURE).  Well-formed and malformed node lists: a child
// count running past the end, a depth over the limit, an unknown op, a null column name, nodes left behind the root, a string
// literal with a length and no bytes, and seeded random lists.  Prints one line per case: name, status, instructions, depth.
// Exit code 0 whenever the compiler RETURNED; a sanitizer report aborts with its own exit code.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../include/orcgpu.h"
#include "../../orc_rust_amd/csrc/orcgpu_filter_plan.inc"

using orcgpu_host::FilterPlan;
using orcgpu_host::filter_compile;

static const char* kNames[] = {"i", "f", "b", "s", "ts", "d", nullptr};
static const int32_t kKinds[] = {ORCGPU_T_LONG, ORCGPU_T_DOUBLE, ORCGPU_T_BOOLEAN, ORCGPU_T_STRING, ORCGPU_T_TIMESTAMP, ORCGPU_T_DATE, ORCGPU_T_INT};

static orcgpu_predicate_node leaf(int op, const char* col, int vt, int64_t i = 0, double f = 0, const char* s = nullptr, uint64_t s_len = 0, int is_null = 0) {
  orcgpu_predicate_node n{};
  n.op = op;
  n.column = col;
  n.value_type = vt;
  n.value_is_null = is_null;
  n.i = i;
  n.f = f;
  n.s = s;
  n.s_len = s_len;
  return n;
}
static orcgpu_predicate_node inner(int op, uint32_t kids) {
  orcgpu_predicate_node n{};
  n.op = op;
  n.n_children = kids;
  return n;
}
static int run(const char* what, const std::vector<orcgpu_predicate_node>& nodes, uint32_t n_columns = 7) {
  FilterPlan plan;
  const int rc = filter_compile(nodes.empty() ? nullptr : nodes.data(), (uint32_t)nodes.size(), kNames, kKinds, n_columns, plan);
  // a program that compiled must run on a stack of kFilterStack slots and leave one word
  long sp = 0, top = 0;
  if (!rc)
    for (auto& in : plan.prog) {
      sp += in.op == FOP_AND || in.op == FOP_OR ? -1 : (in.op == FOP_NOT ? 0 : 1);
      if (sp > top) top = sp;
      if (in.op <= FOP_IS_NOT_NULL && in.col >= n_columns) abort();
      if (in.op == FOP_CMP_STRING && in.lit_off + in.lit_len > plan.lits.size()) abort();
    }
  if (!rc && (sp != 1 || top > (long)kFilterStack || top > (long)plan.depth)) abort();
  printf("%s %d %zu %u\n", what, rc, plan.prog.size(), plan.depth);
  return rc;
}

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1;
  const int n_random = argc > 2 ? atoi(argv[2]) : 2000;
  run("leaf", {leaf(ORCGPU_PRED_EQ, "i", ORCGPU_PV_INT8, 3)});
  run("and3", {inner(ORCGPU_PRED_AND, 3), leaf(ORCGPU_PRED_LT, "f", ORCGPU_PV_FLOAT32, 0, 0.1), leaf(ORCGPU_PRED_IS_NULL, "ts", 0),
               leaf(ORCGPU_PRED_GE, "s", ORCGPU_PV_UTF8, 0, 0, "mango", 5)});
  run("empty_and", {inner(ORCGPU_PRED_AND, 0)});
  run("empty_or", {inner(ORCGPU_PRED_OR, 0)});
  run("null_literal", {leaf(ORCGPU_PRED_EQ, "d", ORCGPU_PV_INT32, 0, 0, nullptr, 0, 1)});
  run("children_past_end", {inner(ORCGPU_PRED_OR, 5), leaf(ORCGPU_PRED_EQ, "i", ORCGPU_PV_INT64, 1)});
  run("children_4_billion", {inner(ORCGPU_PRED_AND, 0xffffffffu), leaf(ORCGPU_PRED_EQ, "i", ORCGPU_PV_INT64, 1)});
  run("not_without_child", {inner(ORCGPU_PRED_NOT, 1)});
  run("left_over", {leaf(ORCGPU_PRED_EQ, "i", ORCGPU_PV_INT64, 1), leaf(ORCGPU_PRED_EQ, "i", ORCGPU_PV_INT64, 2)});
  run("unknown_op", {leaf(11, "i", ORCGPU_PV_INT64, 1)});
  run("negative_op", {leaf(-1, "i", ORCGPU_PV_INT64, 1)});
  run("null_column", {leaf(ORCGPU_PRED_EQ, nullptr, ORCGPU_PV_INT64, 1)});
  run("null_column_null_test", {leaf(ORCGPU_PRED_IS_NOT_NULL, nullptr, 0)});
  run("unknown_column", {leaf(ORCGPU_PRED_EQ, "nope", ORCGPU_PV_INT64, 1)});
  run("no_columns", {leaf(ORCGPU_PRED_EQ, "i", ORCGPU_PV_INT64, 1)}, 0);
  run("type_pair", {leaf(ORCGPU_PRED_EQ, "s", ORCGPU_PV_INT32, 1)});
  run("bad_value_type", {leaf(ORCGPU_PRED_EQ, "i", 99, 1)});
  run("timestamp_compare", {leaf(ORCGPU_PRED_LT, "ts", ORCGPU_PV_INT64, 1)});
  run("string_len_no_bytes", {leaf(ORCGPU_PRED_EQ, "s", ORCGPU_PV_UTF8, 0, 0, nullptr, 9)});
  run("no_nodes", {});
  for (uint32_t d : {ORCGPU_FILTER_MAX_DEPTH, ORCGPU_FILTER_MAX_DEPTH + 1, 100000}) {
    std::vector<orcgpu_predicate_node> chain(d - 1, inner(ORCGPU_PRED_NOT, 1));
    chain.push_back(leaf(ORCGPU_PRED_EQ, "b", ORCGPU_PV_BOOLEAN, 1));
    run(d <= ORCGPU_FILTER_MAX_DEPTH ? "depth_at_limit" : "depth_over_limit", chain);
    std::vector<orcgpu_predicate_node> right;  // AND(x, AND(x, ...)): the stack need grows with the depth
    for (uint32_t k = 0; k + 1 < d; k++) {
      right.push_back(inner(ORCGPU_PRED_AND, 2));
      right.push_back(leaf(ORCGPU_PRED_IS_NULL, "f", 0));
    }
    right.push_back(leaf(ORCGPU_PRED_IS_NULL, "f", 0));
    run(d <= ORCGPU_FILTER_MAX_DEPTH ? "right_deep_at_limit" : "right_deep_over_limit", right);
  }
  std::mt19937 rng(seed);
  int ok = 0;
  const char* cols[] = {"i", "f", "b", "s", "ts", "d", "nope", nullptr};
  for (int k = 0; k < n_random; k++) {
    std::vector<orcgpu_predicate_node> nodes(1 + rng() % 12);
    for (auto& n : nodes) {
      const unsigned roll = rng() % 10;
      if (roll < 3) n = inner(ORCGPU_PRED_AND + (int)(rng() % 3), rng() % 4);
      else n = leaf((int)(rng() % 13) - 1, cols[rng() % 8], (int)(rng() % 9), (int64_t)rng() - 5, 0.5, roll == 9 ? nullptr : "mango", rng() % 6, rng() % 7 == 0);
    }
    FilterPlan plan;
    ok += filter_compile(nodes.data(), (uint32_t)nodes.size(), kNames, kKinds, 7, plan) == 0;
  }
  printf("random %d %d\n", n_random, ok);
  return 0;
}
