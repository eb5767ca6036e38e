"""Division in an expression under AddressSanitizer + UBSan on the CPU: tests/hostcheck/div_check.cpp compiles
orc_rust_amd/csrc/orcgpu_agg_expr.inc (through orcgpu_computed_plan.inc) and device/agg_expr_eval.h -- the text liborcgpu.so is
built from -- into a stand-alone program.  The checked divide against tests/div_model.py on hand vectors (magnitudes of both
operands on either side of 2^32, 2^64 and 2^96, +-1, the 128-bit extremes, 38-digit Decimals, every k, zero divisors, exact halves)
and seeded pairs; the double division against numpy; the plans, the reversed order, the slots, the folding, the class change,
every refusal with its status and message fragment; the interpreter at the edges.  The double division is compared bit for bit,
a NaN's sign and payload included.  No GPU, nothing loaded into Python."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import div_model as M
from orc_rust_amd.aggregate import col, divide, year

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, MISMATCHED, UNSUPPORTED, INVALID = 0, 6, 7, 101
INT, DEC, FLOAT = 0, 1, 2
GATE, PUSH_INT, PUSH_DEC, PUSH_F64, PUSH_LIT, ADD, SUB, MUL, SCALE10, DATE_PART, DIV, FLOOR_DIV, MOD, SWAP = 0, 1, 2, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14, 15
AK_EXPR_INT, AK_EXPR_DEC, AK_EXPR_F64 = 11, 12, 13
ROUND, FLOOR, MODULO = 0, 1, 2
I128_MIN, I128_MAX = -2 ** 127, 2 ** 127 - 1
SCHEMA = {"a": "int", "b": "int", "i": "int", "d": "date", "p": ("dec", 2), "q": ("dec", 4)}
# magnitudes on either side of 2^32, 2^64 and 2^96, +-1, the extremes, 38-digit Decimals
MAGS = [1, 2, 3, 10, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1, 2 ** 64, 2 ** 64 + 1, 2 ** 64 + 2 ** 32, 2 ** 96 - 1, 2 ** 96, 2 ** 96 + 1, 2 ** 126, 10 ** 38 - 1,
        10 ** 37 + 1, 99999999999999999999999999999999999999 // 7, 2 ** 127 - 1]
HAND = [0, I128_MIN, I128_MIN + 1] + MAGS + [-m for m in MAGS]
# (name, the expression for the program, the same for the model, the row)
EVALS = [
    ("unit_price", "/ c:p c:a", col("p") / col("a"), {"p": 1234567, "a": 7}),
    ("half_up", "/:0 c:a c:b", divide("a", "b", scale=0), {"a": 5, "b": 2}),
    ("half_down", "/:0 c:a c:b", divide("a", "b", scale=0), {"a": -5, "b": 2}),
    ("zero_divisor", "/ c:a c:b", col("a") / col("b"), {"a": 5, "b": 0}),
    ("zero_by_zero", "% c:a c:b", col("a") % col("b"), {"a": 0, "b": 0}),
    ("product_leaves_128", "/:38 c:a c:b", divide("a", "b", scale=38), {"a": 2 ** 62, "b": 2 ** 62}),
    ("min_by_minus_one", "// * * c:a c:a i:-2 c:b", (col("a") * col("a") * -2) // col("b"), {"a": 2 ** 63, "b": -1}),
    ("min_mod_minus_one", "% * * c:a c:a i:-2 c:b", (col("a") * col("a") * -2) % col("b"), {"a": 2 ** 63, "b": -1}),
    ("floor_negative", "// c:a c:b", col("a") // col("b"), {"a": -7, "b": 2}),
    ("mod_negative_divisor", "% c:a c:b", col("a") % col("b"), {"a": 7, "b": -2}),
    ("reversed", "// c:a + c:b c:i", col("a") // (col("b") + col("i")), {"a": 100, "b": 3, "i": 4}),
    ("null_operand", "/ c:a c:b", col("a") / col("b"), {"a": 5, "b": None}),
    ("null_beside_zero", "/ c:a + c:b c:i", col("a") / (col("b") + col("i")), {"a": None, "b": 0, "i": 0}),
    ("overflow_then_arithmetic", "* i:0 // c:a c:b", 0 * (col("a") // col("b")), {"a": 1, "b": 0}),
    ("year_mod_times_decimal", "* % year c:d i:100 c:p", year("d") % 100 * col("p"), {"d": 9131, "p": 150}),
    ("wide_divisor", "/:0 * * c:a c:a c:a * c:b c:b", divide(col("a") * col("a") * col("a"), col("b") * col("b"), scale=0), {"a": 2 ** 41 + 3, "b": 2 ** 40 + 1}),
    ("int64_result_leaves_int64", "// c:a c:b", col("a") // col("b"), {"a": -2 ** 63, "b": -1}),
]


def chain(n_plus):
    return " ".join(["+"] * n_plus + ["c:a"] * (n_plus + 1))


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("div_host")
    exe = str(tmp / "div_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "div_check.cpp")])
    rnd = random.Random(20261021)
    vectors = [(mode, a, b, 0) for a in HAND for b in HAND for mode in (ROUND, FLOOR, MODULO)]
    vectors += [(ROUND, a, b, k) for k in range(39) for a, b in ((1, 3), (-2, 3), (10 ** 38 - 1, 7), (5, 10 ** (k + 1)), (-5, 10 ** (k + 1)), (2 ** 126 // 10 ** k, -3), (2 ** 127 // 10 ** k + 1, 1))]
    vectors += [(ROUND, h * d + s * (d // 2), s2 * d, 0) for d in (2, 10, 2 ** 32, 2 ** 64, 2 ** 64 + 2, 2 ** 100) for h in (0, 1, 2 ** 20 + 1) for s in (1, -1) for s2 in (1, -1)]  # exact halves
    for _ in range(6000):
        ba, bb = rnd.choice((20, 40, 63, 64, 65, 96, 100, 127)), rnd.choice((1, 8, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127))
        a, b = rnd.getrandbits(ba) * rnd.choice((1, -1)), rnd.getrandbits(bb) * rnd.choice((1, -1))
        vectors.append((rnd.choice((ROUND, FLOOR, MODULO)), a, b, 0))
        vectors.append((ROUND, a, b, rnd.randint(0, 38)))
    vectors = [v for v in vectors if M.fits(v[1]) and M.fits(v[2])]  # (the operands are int128; a * 10^k may leave it)
    with open(str(tmp / "div.txt"), "w") as f:
        f.write("\n".join("%d %d %d %d" % v for v in vectors))
    specials = [0.0, -0.0, 1.0, -3.0, 0.1, 1e308, 5e-324, float("inf"), float("-inf"), float("nan"), 2.0 ** 53 + 2]
    doubles = [(x, y) for x in specials for y in specials] + [tuple(struct.unpack("<dd", struct.pack("<QQ", rnd.getrandbits(64), rnd.getrandbits(64)))) for _ in range(2000)]
    with open(str(tmp / "fdiv.txt"), "w") as f:
        f.write("\n".join("%x %x" % struct.unpack("<QQ", struct.pack("<dd", x, y)) for x, y in doubles))
    args = ["plan", "nodes_32", "// neg %s i:3" % chain(14), "plan", "nodes_33", "// %s i:3" % chain(15)]
    for name, text, _, row in EVALS:
        args += ["eval", name, text] + ["%s=%d" % (k, v) for k, v in row.items() if v is not None]
    run = subprocess.run([exe, str(tmp / "div.txt"), str(tmp / "fdiv.txt")] + args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    got = {"vectors": vectors, "doubles": doubles}
    for ln in run.stdout.splitlines():
        head, _, msg = ln.partition("\t")
        f = head.split()
        got[(f[0], f[1])] = (f[2:], msg)
    return got


def plan(out, name):
    """status, class, scale, [(op, col, lo)], message"""
    f, msg = out[("plan", name)]
    if int(f[0]) != OK:
        return int(f[0]), None, None, None, msg
    return int(f[0]), int(f[1]), int(f[2]), [tuple(int(x) for x in o.split(":")) for o in f[4:]], msg


def test_the_checked_divide_is_the_models(out):
    assert len(out["vectors"]) > 15000
    paths = set()
    for n, (mode, a, b, k) in enumerate(out["vectors"]):
        f, _ = out[("div", str(n))]
        want = M.div_round(a, b, k) if mode == ROUND else M.floor_div(a, b) if mode == FLOOR else M.mod(a, b)
        assert (int(f[0]), int(f[1])) == ((0, 0) if want is None else (1, want)), (mode, a, b, k)
        if b and M.fits(a * 10 ** k):
            paths.add((abs(a * 10 ** k) >= 2 ** 64, abs(b) >= 2 ** 64))
    assert len(paths) == 4  # both narrow; a wide dividend over a narrow divisor; a wide divisor (under a narrow dividend too)


def test_the_double_division_is_numpys(out):
    a = np.array([x for x, _ in out["doubles"]], dtype=np.float64)
    b = np.array([y for _, y in out["doubles"]], dtype=np.float64)
    with np.errstate(all="ignore"):
        want = a / b
    for n, w in enumerate(want.tolist()):
        assert int(out[("fdiv", str(n))][0][0], 16) == struct.unpack("<Q", struct.pack("<d", w))[0], out["doubles"][n]  # (a NaN's sign and payload too)


def test_the_plans_and_the_class_change(out):
    # int / int is a Decimal at scale 6: the dividend times 10^6
    assert plan(out, "int_by_int")[:4] == (OK, DEC, 6, [(GATE, 0, 0), (GATE, 1, 0), (PUSH_INT, 0, 0), (PUSH_INT, 1, 0), (DIV, 6, 10 ** 6)])
    assert M.computed_type(col("a") / col("b"), SCHEMA) == ("decimal128", 6)
    assert plan(out, "dec_by_int")[1:4] == (DEC, 6, [(GATE, 4, 0), (GATE, 0, 0), (PUSH_DEC, 4, 0), (PUSH_INT, 0, 0), (DIV, 4, 10 ** 4)])
    assert plan(out, "dec_by_dec")[1:3] == (DEC, 6) and plan(out, "dec_by_dec")[3][-1] == (DIV, 8, 10 ** 8)
    assert plan(out, "scale_0")[1:3] == (DEC, 0) and plan(out, "scale_0")[3][-1] == (DIV, 0, 1)
    assert plan(out, "scale_38")[1:3] == (DEC, 38) and plan(out, "scale_38")[3][-1] == (DIV, 38, 10 ** 38)
    assert plan(out, "high_scale_default")[1:3] == (DEC, 38) and plan(out, "high_scale_default")[3][-1] == (DIV, 2, 100)  # min(38, 36 + 4)
    assert plan(out, "floor")[:4] == (OK, INT, 0, [(GATE, 0, 0), (GATE, 2, 0), (PUSH_INT, 0, 0), (PUSH_INT, 2, 0), (FLOOR_DIV, 0, 0)])
    assert plan(out, "mod")[:4] == (OK, INT, 0, [(GATE, 3, 0), (PUSH_INT, 3, 0), (PUSH_LIT, 0, 7), (MOD, 0, 0)])
    assert plan(out, "int_stays_int")[1:3] == (INT, 0)
    assert plan(out, "mod_in_dec")[1:4] == (DEC, 2, [(GATE, 3, 0), (GATE, 4, 0), (PUSH_INT, 3, 0), (DATE_PART, 0, 0), (PUSH_LIT, 0, 100), (MOD, 0, 0), (PUSH_DEC, 4, 0), (MUL, 0, 0)])
    # a quotient at scale 6 plus a Decimal at scale 4: the sum's scale rule is the old one
    assert plan(out, "sum_of_quotients")[1:3] == (DEC, 6) and plan(out, "sum_of_quotients")[3][-4:] == [(DIV, 4, 10 ** 4), (PUSH_DEC, 5, 0), (SCALE10, 2, 100), (ADD, 0, 0)]
    assert plan(out, "float")[:4] == (OK, FLOAT, 0, [(GATE, 6, 0), (GATE, 7, 0), (PUSH_F64, 6, 0), (PUSH_F64, 7, 0), (DIV, 0, 0)])
    assert plan(out, "float_scale_unread")[:2] == (OK, FLOAT) and plan(out, "float_scale_unread")[3][-1] == (DIV, 0, 0)
    assert plan(out, "year_of_integer_quotient")[1:3] == (DEC, 0)


def test_the_reversed_order_is_one_swap(out):
    for name, op, lo in (("reversed_div", DIV, (6, 10 ** 6)), ("reversed_floor", FLOOR_DIV, (0, 0)), ("reversed_mod", MOD, (0, 0))):
        assert plan(out, name)[3][3:] == [(PUSH_INT, 1, 0), (PUSH_INT, 2, 0), (ADD, 0, 0), (PUSH_INT, 0, 0), (SWAP, 0, 0), (op,) + lo], name
    assert plan(out, "reversed_float")[3][2:] == [(PUSH_F64, 7, 0), (PUSH_F64, 7, 0), (MUL, 0, 0), (PUSH_F64, 6, 0), (SWAP, 0, 0), (DIV, 0, 0)]
    assert SWAP not in [o[0] for o in plan(out, "not_reversed")[3]] and plan(out, "not_reversed")[3][-1] == (DIV, 6, 10 ** 6)


def test_the_slots_the_depth_count_and_the_node_limit(out):
    status, cls, scale, ops, _ = plan(out, "deep_4")
    assert (status, cls, scale) == (OK, DEC, 10) and len(ops) == 2 + 15 and ops[-1] == (DIV, 10, 10 ** 10)
    status, _, _, _, msg = plan(out, "deep_5")
    assert status == UNSUPPORTED and "more than ORCGPU_AGG_EXPR_MAX_DEPTH (4) operand slots" in msg
    assert plan(out, "nodes_32")[0] == OK and plan(out, "nodes_32")[3][-1] == (FLOOR_DIV, 0, 0)
    status, _, _, _, msg = plan(out, "nodes_33")
    assert status == INVALID and "more than ORCGPU_AGG_EXPR_MAX_NODES (32) nodes" in msg


def test_literals_fold_with_the_evaluators_functions_unless_they_overflow(out):
    assert plan(out, "folded_div")[3] == [(GATE, 4, 0), (PUSH_DEC, 4, 0), (SCALE10, 4, 10 ** 4), (PUSH_LIT, 0, M.div_round(1, 3, 6)), (ADD, 0, 0)]
    assert plan(out, "folded_half")[3] == [(GATE, 0, 0), (PUSH_INT, 0, 0), (PUSH_LIT, 0, -3), (ADD, 0, 0)] and M.div_round(-5, 2) == -3
    assert plan(out, "folded_floor_mod")[3] == [(GATE, 0, 0), (PUSH_INT, 0, 0), (PUSH_LIT, 0, -7 // 2 + -7 % 2), (ADD, 0, 0)]
    bits = lambda x: struct.unpack("<q", struct.pack("<d", x))[0]
    assert plan(out, "folded_float")[3][2] == (PUSH_LIT, 0, bits(1.0 / 3.0)) and plan(out, "folded_float_zero")[3][2] == (PUSH_LIT, 0, bits(float("inf")))
    # a folding that would overflow is left to the rows
    assert plan(out, "not_folded_zero")[3] == [(GATE, 0, 0), (PUSH_LIT, 0, 1), (PUSH_LIT, 0, 0), (FLOOR_DIV, 0, 0), (PUSH_INT, 0, 0), (ADD, 0, 0)]
    assert plan(out, "not_folded_mod_zero")[3][1:4] == [(PUSH_LIT, 0, 1), (PUSH_LIT, 0, 0), (MOD, 0, 0)]
    assert plan(out, "not_folded_div_zero")[3][1:4] == [(PUSH_LIT, 0, 150), (PUSH_LIT, 0, 0), (DIV, 4, 10 ** 4)]
    assert plan(out, "not_folded_product")[3][1:4] == [(PUSH_LIT, 0, 2 ** 63 - 1), (PUSH_LIT, 0, 3), (DIV, 38, 10 ** 38)]


def test_every_refusal(out):
    for name, code, words in (("bad_scale_39", INVALID, ("names no result scale",)),
                              ("bad_scale_minus_2", INVALID, ("names no result scale",)),
                              ("k_negative", UNSUPPORTED, ("dividend scale 4", "divisor scale 0", "result scale 1", "column 'q'")),
                              ("k_past_38", UNSUPPORTED, ("dividend scale 2", "divisor scale 38", "result scale 6")),
                              ("floor_of_decimal", MISMATCHED, ("// in the expression", "column 'p'", "takes integers")),
                              ("mod_by_decimal", MISMATCHED, ("% in the expression", "column 'a'", "takes integers")),
                              ("mod_of_quotient", MISMATCHED, ("% in the expression", "column 'a'", "non-zero scale")),
                              ("floor_in_float", MISMATCHED, ("Float / Double expression", "column 'x'", "holds //")),
                              ("mod_in_float", MISMATCHED, ("Float / Double expression", "holds %")),
                              ("float_beside_exact", MISMATCHED, ("mixes the Float / Double column 'x' with the integer or Decimal column 'a'",)),
                              ("string_operand", UNSUPPORTED, ("column 's' cannot stand in the expression of computed column 'r'",)),
                              ("year_of_quotient", MISMATCHED, ("year()", "takes days, an integer", "quotient")),
                              ("no_operand", INVALID, ("ends before an operator has its operands",)),
                              ("unknown_20", INVALID, ("an unknown node",))):
        status, _, _, _, msg = plan(out, name)
        assert status == code and all(w in msg for w in words), (name, status, msg)


def test_the_aggregates_mode_and_a_filter_leafs_two_sides(out):
    def agg(name):
        f, msg = out[("agg", name)]
        return int(f[0]), int(f[1]), int(f[2]), int(f[3]), msg
    assert agg("sum_unit_price")[:4] == (OK, AK_EXPR_DEC, 6, 5) and agg("sum_int_quotient")[:3] == (OK, AK_EXPR_DEC, 6)
    assert agg("sum_mod")[:3] == (OK, AK_EXPR_INT, 0) and agg("sum_float")[:3] == (OK, AK_EXPR_F64, 0)
    assert agg("date_outside")[0] == MISMATCHED and "does not take column 'd'" in agg("date_outside")[4]  # outside a date part a Date stays refused
    assert agg("literals_alone")[0] == INVALID and "holds no column" in agg("literals_alone")[4]

    def pair(name):
        f, msg = out[("pair", name)]
        return tuple(int(x) for x in f), msg
    assert pair("quotient_against_int")[0] == (OK, DEC, 6, 0, 5, 1) and pair("int_against_quotient")[0] == (OK, DEC, 0, 6, 2, 4)
    assert pair("mod_against_int")[0] == (OK, INT, 0, 0, 4, 1) and pair("float_pair")[0][:2] == (OK, FLOAT)
    assert pair("floor_beside_float")[0][0] == MISMATCHED


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
    assert want["unit_price"] == (1763667143, False) and want["half_up"] == (3, False) and want["half_down"] == (-3, False)
    assert want["zero_divisor"] == (None, True) and want["zero_by_zero"] == (None, True) and want["product_leaves_128"] == (None, True)
    assert want["min_by_minus_one"] == (None, True) and want["min_mod_minus_one"] == (0, False)
    assert want["floor_negative"] == (-4, False) and want["mod_negative_divisor"] == (-1, False) and want["reversed"] == (14, False)
    assert want["null_operand"] == (None, False) and want["null_beside_zero"] == (None, False)
    assert want["overflow_then_arithmetic"] == (None, True)  # never a wrapped, clamped or silent value, even times zero
    assert want["year_mod_times_decimal"] == (95 * 150, False) and want["int64_result_leaves_int64"] == (None, True)
    assert want["wide_divisor"] == (M.div_round((2 ** 41 + 3) ** 3, (2 ** 40 + 1) ** 2), False) and (2 ** 40 + 1) ** 2 > 2 ** 64
