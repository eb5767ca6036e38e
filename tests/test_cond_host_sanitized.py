"""The conditionals of an expression under AddressSanitizer + UBSan on the CPU: tests/hostcheck/cond_check.cpp compiles
orc_rust_amd/csrc/orcgpu_agg_expr.inc (through orcgpu_computed_plan.inc) and device/agg_expr_eval.h -- the text liborcgpu.so is
built from -- into a stand-alone program.  The plans (no gates and nullable pushes with a conditional, the old op list without),
the scale alignment in CMP / IF / COALESCE, the NULL literal, the ternary node's slots at the limit and past it, every refusal with
its status and a message fragment, a filter leaf's two sides, the bit masks with four slots in use, and the interpreter against
tests/cond_model.py on rows that hold the guard cases.  No GPU, nothing loaded into Python."""
import os
import struct
import subprocess

import pytest

import cond_model as M
from orc_rust_amd import aggregate as A
from orc_rust_amd.aggregate import abs_, case, coalesce, col, lit, nullif, when, year
from orc_rust_amd.predicate import Predicate as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, MISMATCHED, UNSUPPORTED, INVALID = 0, 6, 7, 101
INT, DEC, FLOAT = 0, 1, 2
GATE, PUSH_INT, PUSH_DEC, PUSH_F64, PUSH_LIT, ADD, SUB, RSUB, MUL, NEG, SCALE10, DATE_PART, DIV, FLOOR_DIV, MOD, SWAP = range(16)
CMP, IS_NULL, AND, OR, NOT, IF, COALESCE, ABS, PUSH_NULL = range(16, 25)
EQ, NE, LT, LE, GT, GE = range(6)
# what stands in front of every program with conditionals, and behind one of the FLOAT class: existing ops, for the interpreters without them
MARK, NAN_TAIL = (MOD, 0, 0), [(PUSH_LIT, 0, 0x7ff8000000000000), (ADD, 0, 0)]
SCHEMA = {"a": "int", "b": "int", "i": "int", "d": "date", "p": ("dec", 2), "q": ("dec", 4), "x": "float", "y": "float"}
SIGN = {A.EXPR_ADD: "+", A.EXPR_SUB: "-", A.EXPR_MUL: "*", A.EXPR_NEG: "neg", A.EXPR_DIV: "/", A.EXPR_FLOOR_DIV: "//", A.EXPR_MOD: "%", A.EXPR_DATE_PART: "year",
        A.EXPR_IF: "if", A.EXPR_COALESCE: "coalesce", A.EXPR_ABS: "abs", A.EXPR_NULL: "null", A.EXPR_IS_NULL: "isnull", A.EXPR_AND: "and", A.EXPR_OR: "or",
        A.EXPR_NOT: "not"}
a, b, i, d, p, q, x, y = (col(n) for n in "abidpqxy")
BIG = 2 ** 63 - 1


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def text(e):
    """an Expr as cond_check's tokens, in pre-order"""
    if e.op == A.EXPR_COLUMN:
        return "c:" + e.column
    if e.op == A.EXPR_LITERAL:
        if e.value_type == A.PV_DECIMAL128:
            return "dec:%d:%d" % e.value
        return "i:%d" % e.value if e.value_type == A.PV_INT64 else "f:%x" % bits(e.value)
    head = "cmp:%d" % e.cmp if e.op == A.EXPR_CMP else SIGN[e.op]
    return " ".join([head] + [text(c) for c in e.children])


square = a * a * a * a  # leaves 128 bits for a = 2^63 - 1
FROWS = [{"x": u, "y": v} for u in (None, 1.0, 3.0, float("nan")) for v in (None, 0.5, 2.5, float("nan"), float("-inf"))]
# (name, expression, rows): the guard cases first
EVALS = [
    ("guard_untaken_branch", when(b.ne(0), a // b, 0), [{"a": 7, "b": 0}, {"a": 7, "b": 2}, {"a": 7, "b": None}, {"a": None, "b": 2}]),
    ("guard_false_and", when(b.ne(0) & (a // b > 2), 1, 0), [{"a": 7, "b": 0}, {"a": 7, "b": 2}, {"a": 7, "b": 3}, {"a": None, "b": 0}, {"a": None, "b": 1}]),
    ("guard_and_other_side", when((a // b > 2) & b.ne(0), 1, 0), [{"a": 7, "b": 0}, {"a": 7, "b": 2}]),
    ("guard_true_or", when(b.eq(0) | (a // b > 2), 1, 0), [{"a": 7, "b": 0}, {"a": 7, "b": 2}, {"a": 7, "b": 3}, {"a": None, "b": 3}]),
    ("overflow_taken_branch", when(b > 0, square, 0), [{"a": BIG, "b": 1}, {"a": BIG, "b": 0}, {"a": 3, "b": 1}]),
    ("overflow_in_condition", when(square > 0, 1, 2), [{"a": BIG}, {"a": 2}, {"a": None}]),
    ("unguarded_and_overflows", when((a // b > 2) & (a > 0), 1, 0), [{"a": 7, "b": 0}, {"a": -7, "b": 0}]),
    ("null_against_overflow", square + b, [{"a": BIG, "b": None}, {"a": BIG, "b": 1}, {"a": 2, "b": 1}]),
    ("is_null_of_overflow", when(P.is_null("b") | (square > 0), 1, 0), [{"a": BIG, "b": None}, {"a": BIG, "b": 1}]),
    ("not_unknown", when(~(a < b), 1, 0), [{"a": 1, "b": 2}, {"a": 2, "b": 1}, {"a": None, "b": 1}]),
    ("coalesce_both_null", coalesce(a, b), [{"a": None, "b": None}, {"a": None, "b": 5}, {"a": 4, "b": None}]),
    ("coalesce_overflowed_first", coalesce(square, 0), [{"a": BIG}, {"a": None}, {"a": 2}]),
    ("coalesce_scales", coalesce(p, a), [{"p": None, "a": 3}, {"p": 125, "a": 3}, {"p": None, "a": BIG * 2 ** 60}]),
    ("cmp_scales", when(p < q, p, q), [{"p": 125, "q": 12499}, {"p": 125, "q": 12501}, {"p": 125, "q": None}]),
    ("if_scales_overflow_that_branch", when(b > 0, a * a, p), [{"a": BIG, "b": 1, "p": 5}, {"a": BIG, "b": 0, "p": 5}]),
    ("null_literal", when(a > 2, None, p), [{"a": 3, "p": 5}, {"a": 1, "p": 5}, {"a": None, "p": 5}]),
    ("nullif_divisor", a / nullif(b, 0), [{"a": 7, "b": 0}, {"a": 7, "b": 2}, {"a": None, "b": 0}]),
    ("abs_min", abs(-(a * a * 2)), [{"a": 2 ** 63}, {"a": 3}, {"a": None}]),
    ("abs_of_difference", abs(a - b), [{"a": 3, "b": 10}, {"a": 10, "b": 3}]),
    ("case_bucket", case([(a < 10, 0), (a < 25, 1)], 2), [{"a": 9}, {"a": 10}, {"a": 25}, {"a": None}]),
    ("year_in_branch", when(d > 0, year(d), 0), [{"d": 9131}, {"d": -5}, {"d": None}]),
    ("reversed_cmp", when(a < (b + i) * 2, 1, 0), [{"a": 1, "b": 1, "i": 1}, {"a": 9, "b": 1, "i": 1}]),
    ("reversed_coalesce", coalesce(a, (b + i) * 2), [{"a": None, "b": 1, "i": 1}, {"a": 9, "b": 1, "i": 1}]),
    ("else_first", when(a > 0, b, (b + i) * (a + i)), [{"a": 1, "b": 2, "i": 3}, {"a": 0, "b": 2, "i": 3}]),
    ("float_when", when(x < y, x, y), [{"x": 1.0, "y": float("nan")}, {"x": float("nan"), "y": 2.0}, {"x": -0.0, "y": 0.0}, {"x": None, "y": 1.0},
                                       {"x": float("inf"), "y": float("-inf")}]),
    ("float_ne_nan", when(x.ne(y), 1.0, 0.0), [{"x": float("nan"), "y": float("nan")}, {"x": 1.0, "y": 1.0}]),
    ("float_abs", abs(x), [{"x": -0.0}, {"x": float("-inf")}, {"x": -float("nan")}, {"x": -2.5}, {"x": None}]),
    ("float_coalesce_div", coalesce(x / y, -1.0), [{"x": 1.0, "y": 0.0}, {"x": None, "y": 0.0}, {"x": 0.0, "y": 0.0}]),
    ("float_null_literal", when(x > 0.0, None, x), [{"x": 1.0}, {"x": -1.0}]),
    # the f64 interpreter's AND / OR / NOT / IS_NULL: Kleene over doubles, with NULL and NaN rows
    ("float_and", when((x < y) & (y < 2.0), x, y), FROWS), ("float_or", when((x < y) | (y < 2.0), x, -y), FROWS),
    ("float_not", when(~(x < y), 1.0, 0.0), FROWS), ("float_is_null", when(P.is_null("x") | P.is_not_null("y") & (y > 0.0), 1.0, x), FROWS),
    ("float_not_is_null", coalesce(when(~P.is_null("x") & ~(x >= y), None, x), y, 7.0), FROWS),
]
# the ternary node needs max(lc, 1 + (la == lb ? la + 1 : max(la, lb))) slots: branches of 2 and 2 give four, of 3 and 3 five
two = a + b                # needs two slots
three = two * (b + i)      # needs three
PLANS = {
    "unchanged": "+ * c:a c:p i:3",
    "if_simple": text(when(a < 5, b, 0)),
    "coalesce_lit": text(coalesce(p, 0)),
    "cmp_align": text(when(p < q, 1, 0)),
    "if_align": text(when(a > 0, p, q)),
    "null_then": text(when(a > 0, None, q)),
    "float_null": text(when(x > 0.0, None, y)),
    "abs_folded": "+ c:a abs i:-5",
    "abs_folded_float": "+ c:x abs f:%x" % bits(-0.0),
    "abs_min_not_folded": "+ c:a abs * * i:%d i:%d i:8" % (-2 ** 62, 2 ** 62),
    "and_or_symmetric": text(when(((b + i) * 2 > a) & (a < (b + i) * 2), 1, 0)),
    "slots_4": text(when(two > 0, two, two)),
    "slots_5": text(when(a > 0, three, three)),
    "nodes_32": text(when(a > 0, a + a + a + a + a + a + a + a + a + a + a + a + a, b)) ,
    # the refusals
    "cond_as_root": "cmp:2 c:a c:b",
    "number_as_cond": "if c:a c:b c:i",
    "cond_as_operand": "+ c:a cmp:2 c:a c:b",
    "cond_in_then": "if cmp:2 c:a c:b isnull c:a c:b",
    "number_under_and": "if and c:a cmp:2 c:a c:b c:a c:b",
    "null_as_root": "null",
    "null_in_sum": "+ c:a null",
    "null_in_cmp": "if cmp:0 c:a null c:a c:b",
    "null_beside_null": "if cmp:2 c:a c:b null null",
    "coalesce_nulls": "+ c:a coalesce null null",
    "bad_cmp": "if cmp:6 c:a c:b c:a c:b",
    "float_beside_exact": text(when(a > 0, x, y)),
    "float_branch_beside_exact": "if cmp:2 c:x c:y c:a c:b",
    "if_two_children": "if cmp:2 c:a c:b c:a",
    "unknown_20": "op:20 c:a c:b",
    "unknown_30": "op:30 c:a c:b",
    "string_operand": "coalesce c:s i:0",
}


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cond_host")
    exe = str(tmp / "cond_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "cond_check.cpp")])
    args = []
    for name, t in PLANS.items():
        args += ["plan", name, t]
    args += ["agg", "sum_when", text(when(a > b, a - b, 0)), "agg", "sum_when_dec", text(when(a > 0, p, q)), "agg", "literals_alone", "if cmp:2 i:1 i:2 i:3 i:4",
             "agg", "date_in_cond", text(when(d > 0, a, b))]
    args += ["pair", "when_against_lit", text(when(a < 5, p, q)), "i:3", "pair", "col_against_abs", "c:a", text(abs(b - i)),
             "pair", "float_pair", text(coalesce(x, 0.0)), "c:y", "pair", "exact_beside_float", text(coalesce(a, 0)), "c:x"]
    for name, e, rows in EVALS:
        for k, row in enumerate(rows):
            args += ["eval", "%s.%d" % (name, k), text(e)]
            args += ["%s=%s" % (c, ("%x" % bits(v)) if SCHEMA[c] == "float" else "%d" % v) for c, v in row.items() if v is not None]
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    got = {}
    for ln in run.stdout.splitlines():
        head, _, msg = ln.partition("\t")
        f = head.split()
        got[(f[0], f[1])] = (f[2:], msg)
    return got


def plan(out, name):
    f, msg = out[("plan", name)]
    if int(f[0]) != OK:
        return int(f[0]), None, None, None, msg
    return int(f[0]), int(f[1]), int(f[2]), [tuple(int(v) for v in o.split(":")) for o in f[4:]], msg


def test_a_program_without_a_new_node_is_the_old_op_list(out):
    assert plan(out, "unchanged")[:4] == (OK, DEC, 2, [(GATE, 0, 0), (GATE, 4, 0), (PUSH_INT, 0, 0), (PUSH_DEC, 4, 0), (MUL, 0, 0), (PUSH_LIT, 0, 300), (ADD, 0, 0)])
    # an ABS of a literal folds with the evaluator's own function, and what is left has no new node: gates again
    assert plan(out, "abs_folded")[3] == [(GATE, 0, 0), (PUSH_INT, 0, 0), (PUSH_LIT, 0, 5), (ADD, 0, 0)]
    assert plan(out, "abs_folded_float")[3] == [(GATE, 6, 0), (PUSH_F64, 6, 0), (PUSH_LIT, 0, 0), (ADD, 0, 0)]
    ops = plan(out, "abs_min_not_folded")[3]  # -2^127 does not fold: the rows report it
    assert ops[-2:] == [(ABS, 0, 0), (ADD, 0, 0)] and GATE not in [o[0] for o in ops] and ops[0] == MARK


def test_a_program_with_a_new_node_has_no_gates_and_nullable_pushes(out):
    assert plan(out, "if_simple")[:4] == (OK, INT, 0, [MARK, (PUSH_INT, 0, 1), (PUSH_LIT, 0, 5), (CMP, LT, 0), (PUSH_INT, 1, 1), (PUSH_LIT, 0, 0), (IF, 0, 0)])
    assert plan(out, "coalesce_lit")[:4] == (OK, DEC, 2, [MARK, (PUSH_DEC, 4, 1), (PUSH_LIT, 0, 0), (COALESCE, 0, 0)])
    for name in ("cmp_align", "if_align", "null_then", "float_null", "and_or_symmetric", "slots_4"):
        assert GATE not in [o[0] for o in plan(out, name)[3]], name


def test_the_scale_alignment_and_the_null_literal(out):
    assert plan(out, "cmp_align")[:4] == (OK, DEC, 0, [MARK, (PUSH_DEC, 4, 1), (SCALE10, 2, 100), (PUSH_DEC, 5, 1), (CMP, LT, 0), (PUSH_LIT, 0, 1), (PUSH_LIT, 0, 0), (IF, 0, 0)])
    assert plan(out, "if_align")[1:4] == (DEC, 4, [MARK, (PUSH_INT, 0, 1), (PUSH_LIT, 0, 0), (CMP, GT, 0), (PUSH_DEC, 4, 1), (SCALE10, 2, 100), (PUSH_DEC, 5, 1), (IF, 0, 0)])
    assert plan(out, "null_then")[1:4] == (DEC, 4, [MARK, (PUSH_INT, 0, 1), (PUSH_LIT, 0, 0), (CMP, GT, 0), (PUSH_NULL, 0, 0), (PUSH_DEC, 5, 1), (IF, 0, 0)])
    assert plan(out, "float_null")[1:3] == (FLOAT, 0) and plan(out, "float_null")[3][4:] == [(PUSH_NULL, 0, 0), (PUSH_F64, 7, 1), (IF, 0, 0)] + NAN_TAIL and plan(out, "float_null")[3][0] == MARK
    assert M.computed_type(when(a > 0, p, q), SCHEMA) == ("decimal128", 4) and M.computed_type(when(a > 0, None, q), SCHEMA) == ("decimal128", 4)


def test_the_order_of_evaluation(out):
    # CMP and COALESCE do not commute: one swap where the right side went first; AND / OR are symmetric and need none
    ops = [o[0] for o in plan(out, "and_or_symmetric")[3]]
    assert ops.count(SWAP) == 1 and ops[ops.index(SWAP) + 1] == CMP and AND in ops


def test_the_ternary_nodes_slots_at_the_limit_and_past_it(out):
    assert plan(out, "slots_4")[0] == OK and plan(out, "slots_4")[3][-1][0] == IF and plan(out, "slots_4")[3][0] == MARK
    status, _, _, _, msg = plan(out, "slots_5")
    assert status == UNSUPPORTED and "more than ORCGPU_AGG_EXPR_MAX_DEPTH (4) operand slots" in msg and "column 'a'" in msg
    assert plan(out, "nodes_32")[0] == OK


def test_every_refusal(out):
    for name, code, words in (("cond_as_root", INVALID, ("CMP in the expression", "column 'a'", "number is wanted: it is a condition")),
                              ("number_as_cond", INVALID, ("a column in the expression", "condition is wanted: it is a number")),
                              ("cond_as_operand", INVALID, ("CMP", "number is wanted")),
                              ("cond_in_then", INVALID, ("IS_NULL", "number is wanted")),
                              ("number_under_and", INVALID, ("a column", "condition is wanted")),
                              ("null_as_root", INVALID, ("NULL in the expression", "outside the value operands of IF and COALESCE")),
                              ("null_in_sum", INVALID, ("NULL in the expression", "column 'a'")),
                              ("null_in_cmp", INVALID, ("NULL in the expression",)),
                              ("null_beside_null", INVALID, ("beside another NULL",)),
                              ("coalesce_nulls", INVALID, ("beside another NULL",)),
                              ("bad_cmp", INVALID, ("a CMP node", "names no comparison")),
                              ("float_beside_exact", MISMATCHED, ("mixes the Float / Double column 'x' with the integer or Decimal column 'a'",)),
                              ("float_branch_beside_exact", MISMATCHED, ("mixes the Float / Double column 'x'",)),
                              ("if_two_children", INVALID, ("ends before an operator has its operands",)),
                              ("unknown_20", INVALID, ("an unknown node",)),
                              ("unknown_30", INVALID, ("an unknown node",)),
                              ("string_operand", UNSUPPORTED, ("column 's' cannot stand in the expression of computed column 'r'",))):
        status, _, _, _, msg = plan(out, name)
        assert status == code and all(w in msg for w in words), (name, status, msg)


def test_the_aggregates_mode_and_a_filter_leafs_two_sides(out):
    def agg(name):
        f, msg = out[("agg", name)]
        return int(f[0]), int(f[1]), int(f[2]), int(f[3]), msg
    assert agg("sum_when")[:4] == (OK, 11, 0, 9) and agg("sum_when_dec")[:3] == (OK, 12, 4)
    assert agg("literals_alone")[0] == INVALID and "holds no column" in agg("literals_alone")[4]
    assert agg("date_in_cond")[0] == MISMATCHED and "does not take column 'd'" in agg("date_in_cond")[4]  # outside a date part a Date stays refused

    def pair(name):
        f, msg = out[("pair", name)]
        return tuple(int(v) for v in f), msg
    assert pair("when_against_lit")[0] == (OK, DEC, 4, 0, 8, 1, 1, 0) and pair("col_against_abs")[0] == (OK, INT, 0, 0, 2, 5, 0, 1)
    assert pair("float_pair")[0][:2] == (OK, FLOAT) and pair("exact_beside_float")[0][0] == MISMATCHED


def test_an_interpreter_without_the_conditionals_never_hands_out_a_value(out):
    """cond_check runs both old instantiations on every program of EVALS that holds a new op: the row must overflow (INT / DEC) or
    the result be NaN (FLOAT); it prints `old-interpreter-gave-a-value` in place of the row's line otherwise"""
    lines = [(k, f) for k, (f, _) in out.items() if k[0] == "eval"]
    assert len(lines) > 150 and not [k for k, f in lines if f[0] == "old-interpreter-gave-a-value"]
    # ... by existing ops alone: the mark in front, and `push NaN, add` behind a program of the FLOAT class
    assert plan(out, "float_null")[3][-2:] == NAN_TAIL and plan(out, "if_simple")[3][-1] == (IF, 0, 0)


def test_the_bit_masks_with_four_slots_in_use(out):
    got = {k[1]: tuple(int(v) for v in f) for k, (f, _) in out.items() if k[0] == "bits"}
    assert got == {"four": (0b1001, 0b0010), "merged": (0b100, 0b001), "swapped": (0b100, 0b010), "pushed": (0b1001, 0b0100), "merged3": (0b10, 0b01),
                   "set": (0b00, 0b10)}


@pytest.mark.parametrize("case_", EVALS, ids=[c[0] for c in EVALS])
def test_the_interpreter_is_the_models(out, case_):
    name, e, rows = case_
    kind = M.computed_type(e, SCHEMA)[0]
    for k, row in enumerate(rows):
        want, over = M.computed_value(e, SCHEMA, {c: row.get(c) for c in SCHEMA})
        f, _ = out[("eval", "%s.%d" % (name, k))]
        assert int(f[0]) == (2 if over else 0 if want is None else 1), (name, row, f, want)
        if want is not None:
            assert (int(f[1], 16) == bits(want)) if kind == "float64" else (int(f[1]) == want), (name, row, f, want)


def test_the_rows_hold_the_guard_cases():
    want = {c[0]: [M.computed_value(c[1], SCHEMA, {n: r.get(n) for n in SCHEMA}) for r in c[2]] for c in EVALS}
    assert want["guard_untaken_branch"] == [(0, False), (3, False), (0, False), (None, False)]  # b NULL: UNKNOWN chooses the else branch
    assert want["guard_false_and"] == [(0, False), (1, False), (0, False), (0, False), (0, False)]
    assert want["guard_and_other_side"] == [(0, False), (1, False)] and want["guard_true_or"] == [(1, False), (1, False), (0, False), (0, False)]
    assert want["overflow_taken_branch"] == [(None, True), (0, False), (81, False)] and want["overflow_in_condition"] == [(None, True), (1, False), (2, False)]
    assert want["unguarded_and_overflows"] == [(None, True), (0, False)]  # overflow AND TRUE overflows; overflow AND FALSE is FALSE
    assert want["null_against_overflow"] == [(None, False), (None, True), (17, False)]
    assert want["coalesce_both_null"] == [(None, False), (5, False), (4, False)] and want["coalesce_overflowed_first"] == [(None, True), (0, False), (16, False)]
    assert want["coalesce_scales"] == [(300, False), (125, False), (None, True)]  # the integer branch times 100 overflows that branch only
    assert want["if_scales_overflow_that_branch"][1] == (5, False) and want["if_scales_overflow_that_branch"][0] == (None, True)
    assert want["nullif_divisor"] == [(None, False), (3500000, False), (None, False)] and want["abs_min"][0] == (None, True)
    assert want["float_ne_nan"] == [(1.0, False), (0.0, False)] and want["null_literal"] == [(None, False), (5, False), (5, False)]
