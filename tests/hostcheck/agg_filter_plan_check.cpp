// agg_filter_plan_check.cpp -- the conditions of an aggregate list (agg(x) FILTER (WHERE ...)) through the plan compilers
// (orc_rust_amd/csrc/orcgpu_agg_plan.inc and orcgpu_filter_plan.inc, the very text liborcgpu.so is built from) under AddressSanitizer +
// UBSan, on the CPU (TEST INFRASTRUCTURE).  A stand-alone program: it builds its cases itself and prints one line per fact,
// "<name> <values ...>"; tests/test_agg_filter_plan_sanitized.py holds the lines to what include/orcgpu.h says.  Exit code 0 when it
// ran through; a sanitizer report aborts with its own exit code.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../include/orcgpu.h"
#include "../../orc_rust_amd/csrc/orcgpu_filter_host.inc"
#include "../../orc_rust_amd/csrc/orcgpu_agg_plan.inc"

using orcgpu_host::AggCol;
using orcgpu_host::AggPlan;
using orcgpu_host::FilterPlan;
typedef std::vector<orcgpu_predicate_node> Nodes;

static AggCol col(int32_t orc_type, uint32_t width, uint32_t scale = 0, bool dict = false) {
  AggCol a;
  a.d.orc_type = orc_type;
  a.d.width = width;
  a.d.is_bool = orc_type == ORCGPU_T_BOOLEAN;
  a.d.dict_out = dict;
  a.d.is_string = !dict && orc_type == ORCGPU_T_STRING;
  a.d.has_present = true;
  a.scale = scale;
  return a;
}
static const char* const kNames[] = {"i64", "f64", "s", "dict", "dec15_2"};
static const AggCol kCols[] = {col(ORCGPU_T_LONG, 8), col(ORCGPU_T_DOUBLE, 8), col(ORCGPU_T_STRING, 0), col(ORCGPU_T_STRING, 4, 0, true), col(ORCGPU_T_DECIMAL, 16, 2)};
static const uint32_t kNc = 5;

// every name and literal is a copy of its own, so that equal conditions never share a pointer
static std::vector<std::string*> g_strings;
static const char* own(const char* s) {
  g_strings.push_back(new std::string(s));
  return g_strings.back()->c_str();
}
static orcgpu_predicate_node node(int32_t op, uint32_t n_children = 0, const char* column = nullptr) {
  orcgpu_predicate_node n;
  memset(&n, 0, sizeof(n));
  n.op = op;
  n.n_children = n_children;
  n.column = column ? own(column) : nullptr;
  return n;
}
static orcgpu_predicate_node cmp_i64(int32_t op, const char* column, int64_t v) {
  orcgpu_predicate_node n = node(op, 0, column);
  n.value_type = ORCGPU_PV_INT64;
  n.i = v;
  return n;
}
static orcgpu_predicate_node cmp_f64(int32_t op, const char* column, double v) {
  orcgpu_predicate_node n = node(op, 0, column);
  n.value_type = ORCGPU_PV_FLOAT64;
  n.f = v;
  return n;
}
static orcgpu_predicate_node utf8(int32_t op, const char* column, const char* text) {
  orcgpu_predicate_node n = node(op, 0, column);
  n.value_type = ORCGPU_PV_UTF8;
  n.s = own(text);
  n.s_len = strlen(text);
  return n;
}
static Nodes in_i64(const char* column, std::vector<int64_t> values, bool with_null = false) {
  Nodes out = {node(ORCGPU_PRED_IN, (uint32_t)values.size() + with_null, column)};
  for (int64_t v : values) out.push_back(cmp_i64(ORCGPU_PRED_LITERAL, nullptr, v));
  if (with_null) {
    out.push_back(cmp_i64(ORCGPU_PRED_LITERAL, nullptr, 0));
    out.back().value_is_null = 1;
  }
  return out;
}
static orcgpu_agg_filter view(const Nodes& n) { return orcgpu_agg_filter{n.empty() ? nullptr : n.data(), (uint32_t)n.size()}; }
static orcgpu_agg_spec spec(uint32_t op, const char* column = nullptr) { return orcgpu_agg_spec{op, column, nullptr}; }

static int compile(const std::vector<orcgpu_agg_spec>& specs, const std::vector<Nodes>& conds, AggPlan& plan) {
  std::vector<orcgpu_agg_filter> filters;
  for (const Nodes& n : conds) filters.push_back(view(n));
  return orcgpu_host::agg_compile(specs.data(), nullptr, filters.data(), (uint32_t)specs.size(), kNames, kCols, kNc, plan);
}
static void print_conds(const char* name, int rc, const AggPlan& plan) {
  printf("%s %d %zu", name, rc, plan.cond_spans.size());
  for (const AggInsn& in : plan.insns) printf(" %u", in.cond);
  printf("\n");
}

// The invariants of a program that holds several predicates: every leaf list entry names an instruction of its op, the planes of
// the instructions that have one are 0 .. n_planes - 1 each once, an IN table lies 8-byte and a LIKE pattern 4-byte aligned inside
// the pool
static bool program_sound(const FilterPlan& p) {
  std::set<long long> planes;
  size_t like = 0, in = 0;
  for (size_t k = 0; k < p.prog.size(); k++) {
    const FilterInsn& x = p.prog[k];
    const bool has_plane = (x.op == FOP_LIKE && x.cmp != LIKE_ALL) || (x.op == FOP_IN && !(x.cmp & IN_NO_TABLE));
    if (!has_plane) continue;
    if (x.i < 0 || x.i >= (long long)p.n_planes() || !planes.insert(x.i).second) return false;
    if (x.lit_off + x.lit_len > p.lits.size() || (x.lit_off & (x.op == FOP_IN ? 7 : 3))) return false;
    const std::vector<uint32_t>& leaves = x.op == FOP_LIKE ? p.like_leaves : p.in_leaves;
    size_t hits = 0;
    for (uint32_t l : leaves) hits += l == k;
    if (hits != 1) return false;
    (x.op == FOP_LIKE ? like : in)++;
  }
  return planes.size() == p.n_planes() && like == p.like_leaves.size() && in == p.in_leaves.size();
}
static uint32_t word_at(const FilterPlan& p, uint64_t off) {
  uint32_t w;
  memcpy(&w, p.lits.data() + off, 4);
  return w;
}

int main() {
  const Nodes A = {cmp_i64(ORCGPU_PRED_GT, "i64", 5)}, A2 = {cmp_i64(ORCGPU_PRED_GT, "i64", 5)}, B = {cmp_i64(ORCGPU_PRED_GT, "i64", 6)},
              C = {cmp_i64(ORCGPU_PRED_GE, "i64", 5)}, none;
  AggPlan plan;
  // identical conditions share an index, different ones do not; a spec without one has 0
  {
    const int rc = compile({spec(ORCGPU_AGG_OP_COUNT_ROWS), spec(ORCGPU_AGG_OP_SUM, "i64"), spec(ORCGPU_AGG_OP_SUM, "i64"), spec(ORCGPU_AGG_OP_COUNT_ROWS),
                            spec(ORCGPU_AGG_OP_MAX, "f64")},
                           {A, A2, B, none, C}, plan);
    print_conds("share", rc, plan);
    printf("share_program %zu %u %u %u %u\n", plan.conds.prog.size(), plan.cond_spans[0].first, plan.cond_spans[1].first, plan.cond_spans[2].first, plan.cond_spans[2].n);
  }
  // a literal that differs in its bytes, a column that differs, a NULL literal: different conditions
  {
    const Nodes s1 = {utf8(ORCGPU_PRED_EQ, "s", "abc")}, s2 = {utf8(ORCGPU_PRED_EQ, "s", "abd")}, s3 = {utf8(ORCGPU_PRED_EQ, "s", "abc")};
    Nodes s4 = {utf8(ORCGPU_PRED_EQ, "s", "abc")};
    s4[0].value_is_null = 1;
    const Nodes f1 = {cmp_f64(ORCGPU_PRED_LT, "f64", 0.0)}, f2 = {cmp_f64(ORCGPU_PRED_LT, "f64", -0.0)};
    const int rc = compile(std::vector<orcgpu_agg_spec>(6, spec(ORCGPU_AGG_OP_COUNT_ROWS)), {s1, s2, s3, s4, f1, f2}, plan);
    print_conds("bytes", rc, plan);
  }
  // AVG is one instruction -- the sum, finished over the count of values -- and carries the condition; the kept-rows instruction
  // the call puts behind the list has none
  {
    const int rc = compile({spec(ORCGPU_AGG_OP_AVG, "i64"), spec(ORCGPU_AGG_OP_AVG, "dec15_2")}, {A, A2}, plan);
    print_conds("avg", rc, plan);
    AggInsn kept{};
    kept.kind = AK_COUNT_ROWS;
    printf("kept_rows %u %zu\n", kept.cond, sizeof(AggInsn));
  }
  // no filters at all: what the older entry points call
  {
    const orcgpu_agg_spec s = spec(ORCGPU_AGG_OP_SUM, "i64");
    const int rc = orcgpu_host::agg_compile(&s, nullptr, nullptr, 1, kNames, kCols, kNc, plan);
    print_conds("null_filters", rc, plan);
  }
  // 64 distinct conditions are accepted, 65 refused
  {
    std::vector<Nodes> conds;
    for (int k = 0; k < 65; k++) conds.push_back({cmp_i64(ORCGPU_PRED_EQ, "i64", k)});
    std::vector<orcgpu_agg_filter> filters;
    for (const Nodes& n : conds) filters.push_back(view(n));
    std::vector<uint32_t> cond_of;
    int rc = orcgpu_host::agg_compile_conds(filters.data(), 64, kNames, kCols, kNc, plan, cond_of);
    printf("conds_64 %d %zu %u %u\n", rc, plan.cond_spans.size(), cond_of[0], cond_of[63]);
    rc = orcgpu_host::agg_compile_conds(filters.data(), 65, kNames, kCols, kNc, plan, cond_of);
    printf("conds_65 %d\t%s\n", rc, plan.err);
    // ... 65 specs that share ONE condition are refused as 65 specs are, 64 accepted with one plane
    std::vector<Nodes> same(65, A);
    rc = compile(std::vector<orcgpu_agg_spec>(64, spec(ORCGPU_AGG_OP_COUNT_ROWS)), std::vector<Nodes>(same.begin(), same.begin() + 64), plan);
    printf("specs_64 %d %zu\n", rc, plan.cond_spans.size());
    rc = compile(std::vector<orcgpu_agg_spec>(65, spec(ORCGPU_AGG_OP_COUNT_ROWS)), same, plan);
    printf("specs_65 %d\t%s\n", rc, plan.err);
  }
  // the row filter's refusals, with its statuses and messages
  {
    int rc = compile({spec(ORCGPU_AGG_OP_COUNT_ROWS)}, {{cmp_i64(ORCGPU_PRED_GT, "nope", 5)}}, plan);
    printf("unknown_column %d\t%s\n", rc, plan.err);
    Nodes deep(ORCGPU_FILTER_MAX_DEPTH, node(ORCGPU_PRED_NOT, 1));
    deep.push_back(cmp_i64(ORCGPU_PRED_GT, "i64", 5));  // 64 NOTs above a leaf: 65 levels
    rc = compile({spec(ORCGPU_AGG_OP_COUNT_ROWS)}, {deep}, plan);
    printf("too_deep %d\t%s\n", rc, plan.err);
    deep.erase(deep.begin());
    rc = compile({spec(ORCGPU_AGG_OP_COUNT_ROWS)}, {deep}, plan);
    printf("deep_64 %d %u\n", rc, plan.conds.depth);
    rc = compile({spec(ORCGPU_AGG_OP_COUNT_ROWS)}, {{utf8(ORCGPU_PRED_EQ, "dict", "x")}}, plan);
    printf("dict_column %d\t%s\n", rc, plan.err);
    rc = compile({spec(ORCGPU_AGG_OP_COUNT, "dict")}, {{node(ORCGPU_PRED_IS_NULL, 0, "dict")}}, plan);  // (the validity alone: allowed, as under the row filter)
    printf("dict_null_test %d\n", rc);
    rc = compile({spec(ORCGPU_AGG_OP_COUNT_ROWS)}, {{cmp_f64(ORCGPU_PRED_GT, "i64", 0.5)}}, plan);
    printf("literal_kind %d\t%s\n", rc, plan.err);
    Nodes left_over = A;
    left_over.push_back(cmp_i64(ORCGPU_PRED_GT, "i64", 5));
    rc = compile({spec(ORCGPU_AGG_OP_COUNT_ROWS)}, {left_over}, plan);
    printf("nodes_left %d\t%s\n", rc, plan.err);
    const orcgpu_agg_filter no_nodes = {nullptr, 3};
    const orcgpu_agg_spec s = spec(ORCGPU_AGG_OP_COUNT_ROWS);
    rc = orcgpu_host::agg_compile(&s, nullptr, &no_nodes, 1, kNames, kCols, kNc, plan);
    printf("count_without_nodes %d\t%s\n", rc, plan.err);
  }
  // the bounds check in front of every launch: a cond past the planes, a span past the program
  {
    compile({spec(ORCGPU_AGG_OP_COUNT_ROWS), spec(ORCGPU_AGG_OP_SUM, "i64")}, {A, B}, plan);
    std::vector<AggInsn> insns = plan.insns;
    const int ok = orcgpu_host::agg_plan_in_bounds(insns, plan.ops, kNc, 2);
    const int fewer_planes = orcgpu_host::agg_plan_in_bounds(insns, plan.ops, kNc, 1);
    insns[0].cond = 3;
    const int past = orcgpu_host::agg_plan_in_bounds(insns, plan.ops, kNc, 2);
    insns[0].cond = 0;
    insns[1].cond = 0;
    const int none_needed = orcgpu_host::agg_plan_in_bounds(insns, plan.ops, kNc);
    printf("bounds %d %d %d %d\n", ok, fewer_planes, past, none_needed);
    printf("span_bounds %d %d %d\n", (int)orcgpu_host::agg_conds_in_bounds(plan.cond_spans, 0, plan.conds.prog.size()),
           (int)orcgpu_host::agg_conds_in_bounds(plan.cond_spans, 1, plan.conds.prog.size()),
           (int)orcgpu_host::agg_conds_in_bounds(plan.cond_spans, 3, plan.conds.prog.size() + 3));
  }
  // a list mixing LIKE, IN and comparison conditions: where the programs, the planes and the literals lie
  {
    const Nodes like = {utf8(ORCGPU_PRED_LIKE, "s", "PROMO%")}, in = in_i64("i64", {1, 2, 3}), cmp = {cmp_f64(ORCGPU_PRED_LT, "f64", 0.5)},
                eq = {utf8(ORCGPU_PRED_EQ, "s", "abc")};
    Nodes both = {node(ORCGPU_PRED_AND, 2)};
    both.push_back(utf8(ORCGPU_PRED_LIKE, "s", "%x_z"));
    const Nodes in2 = in_i64("i64", {7, 8}, true);
    both.insert(both.end(), in2.begin(), in2.end());
    const int rc = compile(std::vector<orcgpu_agg_spec>(6, spec(ORCGPU_AGG_OP_COUNT_ROWS)), {like, in, cmp, eq, both, like}, plan);
    print_conds("mixed", rc, plan);
    const FilterPlan& p = plan.conds;
    printf("mixed_spans");
    for (const AggCondSpan& sp : plan.cond_spans) printf(" %u+%u", sp.first, sp.n);
    printf("\n");
    printf("mixed_ops");
    for (const FilterInsn& x : p.prog) printf(" %u", x.op);
    printf("\n");
    printf("mixed_planes %zu  %lld %lld %lld %lld\n", p.n_planes(), p.prog[0].i, p.prog[1].i, p.prog[4].i, p.prog[5].i);
    printf("mixed_leaves like");
    for (uint32_t l : p.like_leaves) printf(" %u", l);
    printf(" in");
    for (uint32_t l : p.in_leaves) printf(" %u", l);
    printf("\n");
    printf("mixed_sound %d\n", (int)program_sound(p));
    // the literals are where the instructions say: the first LIKE's shape, the string EQ's bytes, the second LIKE's shape, the IN tables' kinds
    printf("mixed_lits %u %.*s %u %u %u %u\n", word_at(p, p.prog[0].lit_off), (int)p.prog[3].lit_len, (const char*)p.lits.data() + p.prog[3].lit_off,
           word_at(p, p.prog[4].lit_off), word_at(p, p.prog[1].lit_off), word_at(p, p.prog[5].lit_off + 8), p.prog[5].cmp & IN_HAS_NULL);
    // ... and behind a row filter that has a LIKE and an IN of its own: what the call lays out
    const std::vector<int32_t> kinds = {ORCGPU_T_LONG, ORCGPU_T_DOUBLE, ORCGPU_T_STRING, ORCGPU_T_STRING, ORCGPU_T_DECIMAL}, params = {3, 3, 3, 3, 2};
    Nodes row = {node(ORCGPU_PRED_OR, 2)};
    row.push_back(utf8(ORCGPU_PRED_LIKE, "s", "a%b"));
    const Nodes row_in = in_i64("i64", {10, 11, 12, 13});
    row.insert(row.end(), row_in.begin(), row_in.end());
    FilterPlan call;
    const int frc = orcgpu_host::filter_compile(row.data(), (uint32_t)row.size(), kNames, kinds.data(), kNc, call, params.data());
    const FilterPlan row_alone = call;
    const uint32_t first = orcgpu_host::filter_plan_append(call, p);
    bool same_front = call.prog.size() == row_alone.prog.size() + p.prog.size() && memcmp(call.prog.data(), row_alone.prog.data(), row_alone.prog.size() * sizeof(FilterInsn)) == 0 &&
                      memcmp(call.lits.data(), row_alone.lits.data(), row_alone.lits.size()) == 0;
    bool same_back = true;
    for (size_t k = 0; k < p.prog.size(); k++) {
      const FilterInsn &a = p.prog[k], &b = call.prog[first + k];
      same_back = same_back && a.op == b.op && a.cmp == b.cmp && a.col == b.col && a.lit_len == b.lit_len;
      if (a.lit_len) same_back = same_back && memcmp(p.lits.data() + a.lit_off, call.lits.data() + b.lit_off, a.lit_len) == 0;
    }
    printf("behind_row_filter %d %u %zu %d %d %d  %lld %lld %lld %lld\n", frc, first, call.n_planes(), (int)same_front, (int)same_back, (int)program_sound(call),
           call.prog[first].i, call.prog[first + 1].i, call.prog[first + 4].i, call.prog[first + 5].i);
    printf("behind_leaves like");
    for (uint32_t l : call.like_leaves) printf(" %u", l);
    printf(" in");
    for (uint32_t l : call.in_leaves) printf(" %u", l);
    printf("\n");
  }
  for (std::string* s : g_strings) delete s;
  return 0;
}
