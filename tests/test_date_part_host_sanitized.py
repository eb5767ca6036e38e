"""The date part of an expression under AddressSanitizer + UBSan on the CPU: tests/hostcheck/date_part_check.cpp compiles
orc_rust_amd/csrc/orcgpu_agg_expr.inc (through orcgpu_computed_plan.inc) and device/agg_expr_eval.h -- the text liborcgpu.so is
built from -- into a stand-alone program.  The calendar function against tests/date_part_model.py on hand days and seeded days
over int32; the plans, the folding, the slots, every refusal with its status and message fragment, the aggregates' mode; the
interpreter at the int32 edges.  No GPU, nothing loaded into Python."""
import os
import random
import subprocess

import pytest

import date_part_model as M
from orc_rust_amd.aggregate import col, day_of_year, month, year

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, MISMATCHED, UNSUPPORTED, INVALID = 0, 6, 7, 101
INT, DEC = 0, 1
GATE, PUSH_INT, PUSH_DEC, PUSH_LIT, ADD, SUB, MUL, DATE_PART = 0, 1, 2, 4, 5, 6, 8, 11
AK_EXPR_INT, AK_EXPR_DEC = 11, 12
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
SCHEMA = {"a": "int", "b": "int", "i": "int", "d": "date", "p": ("dec", 2)}
HAND = [I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX, 11016, 11017, -25508, -25507, -135081, -135080, -719528, -719529, -719468, -719469,
        10957, 10956, 146096, 146097, -146097, -146098]
# (name, the expression for the program, the same for the model, the row)
EVALS = [
    ("max", "year c:d", year("d"), {"d": I32_MAX}),
    ("min", "year c:d", year("d"), {"d": I32_MIN}),
    ("max_plus_1", "year + c:d c:a", year(col("d") + col("a")), {"d": I32_MAX, "a": 1}),
    ("min_minus_1", "doy - c:d c:a", day_of_year(col("d") - col("a")), {"d": I32_MIN, "a": 1}),
    ("long_in_range", "month c:a", month("a"), {"a": I32_MIN}),
    ("long_past", "month c:a", month("a"), {"a": 2 ** 40}),
    ("operand_leaves_128", "year * * c:a c:a c:a", year(col("a") * col("a") * col("a")), {"a": 2 ** 62}),
    ("null_operand", "year + c:d c:a", year(col("d") + col("a")), {"d": 5, "a": None}),
    ("null_beside_overflow", "year + c:d c:a", year(col("d") + col("a")), {"d": None, "a": 2 ** 62}),
    ("yyyymm", "+ * year c:d i:100 month c:d", year("d") * 100 + month("d"), {"d": 9131}),
    ("times_decimal", "* year c:d c:p", year("d") * col("p"), {"d": 0, "p": 150}),
    ("overflow_then_arithmetic", "* i:0 year c:a", 0 * year("a"), {"a": 2 ** 31}),
]


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("date_part_host")
    exe = str(tmp / "date_part_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "date_part_check.cpp")])
    rnd = random.Random(20261021)
    days = HAND + [rnd.randint(I32_MIN, I32_MAX) for _ in range(4000)] + [rnd.randint(-800000, 3000000) for _ in range(1000)]
    with open(str(tmp / "days.txt"), "w") as f:
        f.write("\n".join(str(d) for d in days))
    args = []
    for name, text, _, row in EVALS:
        args += ["eval", name, text] + ["%s=%d" % (k, v) for k, v in row.items() if v is not None]
    run = subprocess.run([exe, str(tmp / "days.txt")] + args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    got = {"days": days}
    for ln in run.stdout.splitlines():
        head, _, msg = ln.partition("\t")
        f = head.split()
        got[(f[0], f[1])] = (f[2:], msg)
    return got


def plan(out, name, kind="plan"):
    """status, class, scale, [(op, col, lo)], message"""
    f, msg = out[(kind, name)]
    if int(f[0]) != OK:
        return int(f[0]), None, None, None, msg
    return int(f[0]), int(f[1]), int(f[2]), [tuple(int(x) for x in o.split(":")) for o in f[4:]], msg


def test_the_calendar_function_is_the_models(out):
    assert len(out["days"]) > 5000
    for d in out["days"]:
        got = tuple(int(x) for x in out[("part", str(d))][0])
        assert got == tuple(M.part_of(d, p) for p in range(6)), d
    assert int(out[("part", str(I32_MIN))][0][0]) == -5877641 and int(out[("part", str(I32_MAX))][0][0]) == 5881580


def test_the_plans(out):
    assert plan(out, "year")[:4] == (OK, INT, 0, [(GATE, 3, 0), (PUSH_INT, 3, 0), (DATE_PART, M.YEAR, 0)])
    status, cls, scale, ops, _ = plan(out, "yyyymm")  # year(d + a) * 100 + month(d)
    assert (status, cls, scale) == (OK, INT, 0)
    assert ops == [(GATE, 3, 0), (GATE, 0, 0), (PUSH_INT, 3, 0), (PUSH_INT, 0, 0), (ADD, 0, 0), (DATE_PART, M.YEAR, 0), (PUSH_LIT, 0, 100), (MUL, 0, 0),
                   (PUSH_INT, 3, 0), (DATE_PART, M.MONTH, 0), (ADD, 0, 0)]
    status, cls, scale, ops, _ = plan(out, "year_times_dec")  # an integer of scale 0 in a Decimal expression: the scale is p's
    assert (status, cls, scale) == (OK, DEC, 2) and ops[2:] == [(PUSH_INT, 3, 0), (DATE_PART, M.YEAR, 0), (PUSH_DEC, 4, 0), (MUL, 0, 0)]
    assert M.computed_type(year("d") * col("p"), SCHEMA) == ("decimal128", 2)
    assert plan(out, "nested")[3][2:] == [(DATE_PART, M.YEAR, 0), (DATE_PART, M.YEAR, 0)]
    assert plan(out, "int_operand")[3][-2:] == [(SUB, 0, 0), (DATE_PART, M.DAY_OF_YEAR, 0)]


def test_a_date_part_of_literals_folds_with_the_evaluators_function(out):
    assert plan(out, "folded")[3] == [(GATE, 0, 0), (PUSH_INT, 0, 0), (PUSH_LIT, 0, M.part_of(9131, M.YEAR)), (ADD, 0, 0)]
    assert plan(out, "folded_all_parts")[3][2] == (PUSH_LIT, 0, sum(M.part_of(-1, p) for p in range(6)))
    # one that overflows is left to the rows
    assert plan(out, "not_folded_overflow")[3] == [(GATE, 0, 0), (PUSH_INT, 0, 0), (PUSH_LIT, 0, 2 ** 31), (DATE_PART, M.YEAR, 0), (ADD, 0, 0)]


def test_the_node_is_unary_for_slots_and_counts_as_a_node(out):
    status, _, _, ops, _ = plan(out, "deep_4")
    assert status == OK and ops[-1] == (DATE_PART, M.YEAR, 0) and len(ops) == 2 + 15 + 1
    status, _, _, _, msg = plan(out, "deep_5")
    assert status == UNSUPPORTED and "more than ORCGPU_AGG_EXPR_MAX_DEPTH (4) operand slots" in msg
    assert plan(out, "nodes_32")[0] == OK
    status, _, _, _, msg = plan(out, "nodes_33")
    assert status == INVALID and "more than ORCGPU_AGG_EXPR_MAX_NODES (32) nodes" in msg


def test_every_refusal(out):
    for name, code, words in (("decimal_below", MISMATCHED, ("year()", "column 'p'", "Decimal")),
                              ("float_below", MISMATCHED, ("month()", "column 'x'", "Float / Double")),
                              ("decimal_literal_below", MISMATCHED, ("year()", "DECIMAL128 literal")),
                              ("float_literal_below", MISMATCHED, ("year()", "FLOAT64 literal")),
                              ("float_expression", MISMATCHED, ("Float / Double expression", "year()")),
                              ("float_column_beside", MISMATCHED, ("mixes the Float / Double column 'x' with the integer or Decimal column 'd'",)),
                              ("string_below", UNSUPPORTED, ("column 's' cannot stand in the expression of computed column 'r'",)),
                              ("boolean_below", UNSUPPORTED, ("column 't' cannot stand in the expression of computed column 'r'",)),
                              ("timestamp_below", UNSUPPORTED, ("column 'ts' cannot stand in the expression of computed column 'r'",)),
                              ("dictionary_below", UNSUPPORTED, ("column 's' is read as a dictionary column",)),
                              ("bad_part", INVALID, ("names no part",)),
                              ("negative_part", INVALID, ("names no part",)),
                              ("no_operand", INVALID, ("ends before an operator has its operands",)),
                              ("unknown_9", INVALID, ("an unknown node",)),
                              ("unknown_15", INVALID, ("an unknown node",))):
        status, _, _, _, msg = plan(out, name)
        assert status == code and all(w in msg for w in words), (name, status, msg)


def test_the_aggregates_mode(out):
    def agg(name):
        f, msg = out[("agg", name)]
        return int(f[0]), int(f[1]), int(f[2]), int(f[3]), msg
    assert agg("sum_year")[:4] == (OK, AK_EXPR_INT, 0, 3)  # below the node a Date is days
    assert agg("sum_year_plus")[:2] == (OK, AK_EXPR_INT)
    assert agg("year_times_dec")[:3] == (OK, AK_EXPR_DEC, 2)
    # outside the node nothing changes
    for name in ("date_plus_1", "date_beside_year"):
        status, _, _, _, msg = agg(name)
        assert status == MISMATCHED and "the expression of SUM_EXPR does not take column 'd'" in msg, name
    for name, column in (("timestamp_below", "ts"), ("string_below", "s")):
        status, _, _, _, msg = agg(name)
        assert status == MISMATCHED and "does not take column '%s'" % column in msg
    status, _, _, _, msg = agg("decimal_below")
    assert status == MISMATCHED and "year()" in msg and "column 'p'" in msg
    assert agg("literals_alone")[0] == INVALID and "holds no column" in agg("literals_alone")[4]


@pytest.mark.parametrize("case", EVALS, ids=[c[0] for c in EVALS])
def test_the_interpreter_at_the_edges(out, case):
    name, _, e, row = case
    want, over = M.computed_value(e, SCHEMA, {k: row.get(k) for k in SCHEMA})
    f, _ = out[("eval", name)]
    assert int(f[0]) == (2 if over else 0 if want is None else 1), (name, f)
    if want is not None:
        assert int(f[1]) == want, (name, f)


def test_the_hand_cases_hold_the_edges():
    want = {c[0]: M.computed_value(c[2], SCHEMA, {k: c[3].get(k) for k in SCHEMA}) for c in EVALS}
    assert want["max"] == (5881580, False) and want["min"] == (-5877641, False)
    assert want["max_plus_1"] == (None, True) and want["min_minus_1"] == (None, True) and want["long_past"] == (None, True)
    assert want["operand_leaves_128"] == (None, True) and want["null_operand"] == (None, False) and want["null_beside_overflow"] == (None, False)
    assert want["yyyymm"] == (199501, False) and want["times_decimal"] == (1970 * 150, False)
    assert want["overflow_then_arithmetic"] == (None, True)  # never a wrapped or clamped value, even times zero
