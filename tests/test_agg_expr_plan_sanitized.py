"""The expression aggregates' plan compiler, the evaluator the kernels run and AVG's division under AddressSanitizer + UBSan on the
CPU: tests/hostcheck/agg_expr_check.cpp compiles orc_rust_amd/csrc/orcgpu_agg_plan.inc, orcgpu_agg_expr.inc and
device/agg_expr_eval.h -- the text liborcgpu.so is built from -- into a stand-alone program.  The class table and every refusal of
include/orcgpu.h with its status and the named column, the scale rule at 38 / 39, four and five operand slots, 32 / 33 nodes, literal
folding; the evaluator against Python ints over random trees and over the edges of 128 bits; the division against Fraction.  No GPU,
nothing loaded into Python."""
import fractions
import os
import subprocess

import numpy as np
import pytest

import agg_expr_model as XM
from orc_rust_amd import aggregate as A
from orc_rust_amd.aggregate import col, lit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, MISMATCHED, UNSUPPORTED, INVALID = 0, 6, 7, 101
AK_SUM_INT, AK_SUM_DEC, AK_SUM_F64, AK_EXPR_INT, AK_EXPR_DEC, AK_EXPR_F64 = 2, 3, 4, 11, 12, 13
KIND_DEC128, KIND_F64 = 2, 3
SUM_EXPR, AVG_EXPR = 6, 8
RNG = np.random.default_rng(41)
I128_MAX, I128_MIN, T38 = 2 ** 127 - 1, -2 ** 127, 10 ** 38
FAMILY = {"i8": "int", "i16": "int", "i32": "int", "i64": "int", "j64": "int", "k64": "int", "f32": "float", "f64": "float", "g64": "float", "dec15_2": "decimal",
          "dec12_5": "decimal", "dec38_0": "decimal", "dec38_19": "decimal", "dec38_20": "decimal", "dec38_38": "decimal"}
SCALE = {"dec15_2": 2, "dec12_5": 5, "dec38_0": 0, "dec38_19": 19, "dec38_20": 20, "dec38_38": 38}


def balanced(leaves):
    if len(leaves) == 1:
        return leaves[0]
    h = len(leaves) // 2
    return balanced(leaves[:h]) + balanced(leaves[h:])


def chain(n_leaves, right=False):
    e = col("i64")
    for _ in range(n_leaves - 1):
        e = (col("i64") - e) if right else (e - col("i64"))
    return e


PLANS = {
    # the class table
    "int": (col("i8") * col("i16") + col("i32") - col("i64") * 3, OK, AK_EXPR_INT, 0),
    "dec_q1": (col("dec15_2") * (1 - col("dec15_2")), OK, AK_EXPR_DEC, 4),
    "dec_q1_tax": (col("dec15_2") * (1 - col("dec15_2")) * (1 + col("dec15_2")), OK, AK_EXPR_DEC, 6),
    "dec_with_int_col": (col("dec15_2") * col("i32") + col("i64"), OK, AK_EXPR_DEC, 2),
    "dec_by_literal": (col("i64") + lit(A.decimal.Decimal("0.125")), OK, AK_EXPR_DEC, 3),
    "dec_align": (col("dec15_2") + col("dec12_5"), OK, AK_EXPR_DEC, 5),
    "dec_neg": (-col("dec12_5"), OK, AK_EXPR_DEC, 5),
    "float": (col("f32") * (1 - col("f64")) + 0.5, OK, AK_EXPR_F64, 0),
    "float_int_lit": (col("f64") * 2 ** 53, OK, AK_EXPR_F64, 0),
    # the scale rule at 38 / 39
    "scale_38": (col("dec38_19") * col("dec38_19"), OK, AK_EXPR_DEC, 38),
    "scale_38_add": (col("dec38_38") + col("i64"), OK, AK_EXPR_DEC, 38),
    "scale_39": (col("dec38_19") * col("dec38_20"), UNSUPPORTED, "dec38_19", None),
    "scale_39_inner": ((col("i64") + col("dec38_20") * col("dec38_19")) - 1, UNSUPPORTED, "i64", None),
    "scale_39_lit": (col("dec38_38") * lit(A.decimal.Decimal("0.1")), UNSUPPORTED, "dec38_38", None),
    # refusals, the message naming the column
    "mix_float_int": (col("f64") + col("i64"), MISMATCHED, "i64", None),
    "mix_float_dec": (col("dec15_2") * col("f32"), MISMATCHED, "dec15_2", None),
    "f64_lit_in_int": (col("i64") * 0.5, MISMATCHED, "i64", None),
    "f64_lit_in_dec": (col("dec15_2") + 0.5, MISMATCHED, "dec15_2", None),
    "dec_lit_in_float": (col("f64") + lit(A.decimal.Decimal("0.5")), MISMATCHED, "f64", None),
    "date": (col("date") + 1, MISMATCHED, "date", None),
    "bool": (col("b") * 2, MISMATCHED, "'b'", None),
    "ts": (col("ts") - 1, MISMATCHED, "'ts'", None),
    "string": (col("i64") + col("s"), MISMATCHED, "'s'", None),
    "narrow_decode": (col("i64_as_i16") + 1, OK, AK_EXPR_INT, 0),          # (a Long decoded to 2 bytes is an integer column like another)
    "dict": (col("dict") + 1, UNSUPPORTED, "dict", None),
    "ts9": (col("ts9") + 1, UNSUPPORTED, "ts9", None),
    "unknown": (col("i64") + col("nope"), INVALID, "nope", None),
    "no_column": (lit(1) + lit(2), INVALID, "no column", None),
    "inexact_int_lit": (col("f64") + (2 ** 53 + 1), INVALID, "f64", None),
    # operand slots: 4 are served, the balanced tree of 16 leaves needs 5
    "balanced_8": (balanced([col("i64")] * 8), OK, AK_EXPR_INT, 0),
    "balanced_16": (balanced([col("i64")] * 16), UNSUPPORTED, "i64", None),
    "balanced_16_two_scales": (balanced([col("dec15_2")] * 8) + balanced([col("dec12_5")] * 8), UNSUPPORTED, "operand slots", None),   # the rescale is unary
    "balanced_16_two_scales_r": (balanced([col("dec12_5")] * 8) - balanced([col("dec15_2")] * 8), UNSUPPORTED, "operand slots", None),
    "balanced_8_two_scales": (balanced([col("dec15_2")] * 4) + balanced([col("dec12_5")] * 4), OK, AK_EXPR_DEC, 5),
    "rescaled_deep_side": ((col("dec15_2") * col("i64") - col("i32") * col("dec15_2")) + (col("dec12_5") + col("dec12_5")), OK, AK_EXPR_DEC, 5),
    "left_chain_16": (chain(16), OK, AK_EXPR_INT, 0),
    "right_chain_16": (chain(16, right=True), OK, AK_EXPR_INT, 0),
    # nodes: 31 fit, the next tree of binary operators has 33
    "nodes_31": (chain(16), OK, AK_EXPR_INT, 0),
    "nodes_32": (-chain(16), OK, AK_EXPR_INT, 0),
    "nodes_33": (chain(17), INVALID, "32", None),
}
RAW = {   # token lists that no Expr builds
    "trailing": ("6 + c:i64 i:1 c:i64", INVALID, "left over"),
    "short": ("6 + c:i64", INVALID, "operands"),
    "short_neg": ("6 neg", INVALID, "operands"),
    "unknown_node": ("6 + c:i64 x:9", INVALID, "unknown node"),
    "bool_literal": ("6 + c:i64 v:0", INVALID, "literal"),
    "utf8_literal": ("6 + c:i64 v:7", INVALID, "literal"),
    "bad_dec_len": ("6 + c:dec15_2 dbad:15:2", INVALID, "dec15_2"),
    "bad_dec_scale": ("6 + dbad:16:39 c:dec15_2", INVALID, "dec15_2"),
    "bad_dec_range": ("6 + c:dec15_2 dbad:16:2", INVALID, "dec15_2"),
    "null_name": ("6 + c:NULL i:1", INVALID, "name"),
    "no_expr": ("6 none", INVALID, "without an expression"),
    "no_expr_avg": ("8 none", INVALID, "without an expression"),
    "empty": ("6", INVALID, "without an expression"),
    "avg_expr": ("8 * c:dec15_2 c:dec15_2", OK, ""),
}
# literal folding: the number of ops of the program (gates included) and its slots
FOLDS = {
    "fold_int": (col("i64") * (lit(2) + lit(3) * lit(4)), 1 + 3, 2),
    "fold_neg": (col("i64") + -lit(5), 1 + 3, 2),
    "fold_dec_rescale": (col("dec12_5") + lit(A.decimal.Decimal("1.5")), 1 + 3, 2),       # 1.5 becomes 150000 at scale 5: no op for it
    "fold_float": (col("f64") * (lit(0.5) + lit(0.25)), 1 + 3, 2),
    "no_fold_overflow": (col("i64") + lit(2 ** 63 - 1) * lit(2 ** 63 - 1) * lit(4), 1 + 5, 2),   # 2^128 does not fit: left to the rows
    "rescale_column": (col("dec15_2") + col("dec12_5"), 2 + 4, 2),                         # push, times 10^3, push, add
    "q1": (col("dec15_2") * (1 - col("dec12_5")), 2 + 5, 2),
}


def rand_value(bits):
    v = int.from_bytes(RNG.bytes(16), "little") >> (128 - bits)
    return -v if RNG.random() < 0.5 else v


def rand_tree(cls, depth):
    cols = {"int": ["i64", "j64", "k64", "i32"], "dec": ["dec15_2", "dec12_5", "dec38_0", "i64"], "float": ["f64", "g64", "f32"]}[cls]
    if depth == 0 or RNG.random() < 0.25:
        if RNG.random() < 0.3:
            if cls == "float":
                return lit(float(RNG.integers(-8, 9)) / 4)
            if cls == "dec" and RNG.random() < 0.5:
                return lit(A.decimal.Decimal(int(RNG.integers(-999, 1000))).scaleb(-int(RNG.integers(0, 4))))
            return lit(int(RNG.integers(-1000, 1000)))
        return col(cols[int(RNG.integers(0, len(cols)))])
    k = int(RNG.integers(0, 7))
    a = rand_tree(cls, depth - 1)
    if k == 0:
        return -a
    b = rand_tree(cls, depth - 1)
    return a + b if k < 3 else a - b if k < 5 else a * b


def rand_evals():
    out = {}
    n = 0
    while len(out) < 300:
        n += 1
        cls = ("int", "dec", "float")[n % 3]
        e = rand_tree(cls, int(RNG.integers(1, 5)))
        names = sorted({x.column for x in XM.leaves(e) if x.op == A.EXPR_COLUMN})
        if not names or e.node_count() > 32 or XM.slots(e) > 4:
            continue
        if cls == "dec" and not any(FAMILY[c] == "decimal" for c in names) and not any(x.value_type == A.PV_DECIMAL128 for x in XM.leaves(e) if x.op == A.EXPR_LITERAL):
            cls = "int"
        try:
            if cls == "dec":
                XM.scale_of(e, SCALE)
        except XM.Refused:
            continue
        row = {}
        for c in names:
            if RNG.random() < 0.05:
                row[c] = None
            elif FAMILY[c] == "float":
                row[c] = float(RNG.integers(-2 ** 20, 2 ** 20)) / 64
            else:
                row[c] = rand_value(int(RNG.integers(1, 31 if c == "i32" else 64 if FAMILY[c] == "int" else 120)))
        out["rand%d" % len(out)] = (e, cls, row)
    return out


X, Y = col("i64"), col("j64")
P = col("dec38_0")
EDGES = {   # (expression, class, row) -> judged by the model
    "neg_2_64_times_2_63": (P * Y, "dec", {"dec38_0": -2 ** 64, "j64": 2 ** 63 - 1}),
    "min_by_product": (X * Y * Y, "int", {"i64": -2 ** 63, "j64": 2 ** 32}),               # exactly -2^127: fits
    "max_plus_1_by_product": (X * Y * Y * -1, "int", {"i64": -2 ** 63, "j64": 2 ** 32}),   # 2^127: does not
    "p_2_64_times_2_63": (P * P, "dec", {"dec38_0": 2 ** 64}),                               # 2^128: does not
    "max_plus_1": (P + 1, "dec", {"dec38_0": I128_MAX}), "max_minus_1": (P - 1, "dec", {"dec38_0": I128_MAX}),
    "min_minus_1": (P - 1, "dec", {"dec38_0": I128_MIN}), "min_plus_1": (P + 1, "dec", {"dec38_0": I128_MIN}),
    "neg_min": (-P, "dec", {"dec38_0": I128_MIN}), "neg_max": (-P, "dec", {"dec38_0": I128_MAX}),
    "sub_min": (0 - P, "dec", {"dec38_0": I128_MIN}), "rsub": (X - (Y * Y + X), "int", {"i64": 5, "j64": 7}),
    "rescale_38_one": (P + col("dec38_38"), "dec", {"dec38_0": 1, "dec38_38": 5}), "rescale_38_two": (P + col("dec38_38"), "dec", {"dec38_0": 2, "dec38_38": 5}),
    "rescale_38_neg": (col("dec38_38") - P, "dec", {"dec38_0": -1, "dec38_38": -7}),
    "null_gate": (X * 2 + Y, "int", {"i64": 3, "j64": None}), "null_first": (X * 2 + Y, "int", {"i64": None, "j64": 3}),
    "float_order": ((col("f64") + col("g64")) * col("f64") - 0.1, "float", {"f64": 0.1, "g64": 0.2}),
    "float_no_fma": (col("f64") * col("g64") + col("f32"), "float", {"f64": 1.0 + 2.0 ** -30, "g64": 1.0 - 2.0 ** -30, "f32": -1.0}),
}
ARITH = [("mul", a, b) for a in (0, 1, -1, 2 ** 63, -2 ** 63, 2 ** 64, -2 ** 64, 2 ** 64 - 1, I128_MAX, I128_MIN, 10 ** 19, -10 ** 19, 3 ** 40)
         for b in (0, 1, -1, 2, -2, 2 ** 63, -2 ** 63, 2 ** 63 - 1, 2 ** 64, I128_MAX, I128_MIN, 10 ** 19)]
ARITH += [(op, a, b) for op in ("add", "sub") for a in (0, 1, -1, I128_MAX, I128_MIN, I128_MAX - 1, I128_MIN + 1) for b in (0, 1, -1, I128_MAX, I128_MIN)]
ARITH += [("neg", a, 0) for a in (0, 1, -1, I128_MAX, I128_MIN, I128_MIN + 1)]
ARITH += [("scale", a, k) for a in (0, 1, -1, 17, -17, I128_MAX // 10 ** 38, I128_MAX // 10 ** 38 + 1, 10 ** 19) for k in (0, 1, 19, 37, 38)]
for _ in range(300):
    _a, _b = rand_value(int(RNG.integers(1, 128))), rand_value(int(RNG.integers(1, 128)))
    ARITH.append((("mul", "add", "sub")[int(RNG.integers(0, 3))], _a, _b))
# AVG: (kind, scale, count, sum)
AVGS = [(AK_SUM_DEC, 2, 3, 1), (AK_SUM_DEC, 2, 3, 2), (AK_SUM_DEC, 2, 3, -2), (AK_SUM_DEC, 0, 20000, 1), (AK_SUM_DEC, 0, 20000, -1), (AK_SUM_DEC, 0, 20001, 1),
        (AK_SUM_DEC, 0, 20000, 3), (AK_SUM_DEC, 0, 20000, -3), (AK_SUM_DEC, 36, 2, 7), (AK_SUM_DEC, 38, 2, 7), (AK_SUM_DEC, 38, 2, -7), (AK_SUM_DEC, 37, 4, 10),
        (AK_EXPR_DEC, 0, 1, T38 - 1), (AK_EXPR_DEC, 0, 1, -(T38 - 1)), (AK_EXPR_DEC, 0, 10 ** 4, T38 - 1), (AK_EXPR_DEC, 0, 10 ** 4 + 1, -(T38 - 1)),
        (AK_EXPR_DEC, 34, 9999, T38 - 1), (AK_EXPR_DEC, 38, 1, T38 - 1), (AK_EXPR_DEC, 2, 2 ** 64 - 1, T38 - 1), (AK_EXPR_DEC, 2, 2 ** 64 - 1, 2 ** 63),
        (AK_EXPR_DEC, 4, 2 ** 63 + 1, -(2 ** 62 + 1) * 10), (AK_SUM_DEC, 0, 7, T38), (AK_SUM_DEC, 0, 7, 0),
        (AK_SUM_INT, 0, 1, 2 ** 53 + 1), (AK_SUM_INT, 0, 1, 2 ** 53 + 3), (AK_SUM_INT, 0, 3, 3 * 2 ** 60 + 1), (AK_SUM_INT, 0, 3, -(3 * 2 ** 60 + 1)),
        (AK_EXPR_INT, 0, 7, I128_MAX), (AK_EXPR_INT, 0, 2 ** 64 - 1, I128_MIN), (AK_EXPR_INT, 0, 2 ** 64 - 1, 1), (AK_EXPR_INT, 0, 2 ** 64 - 1, 2 ** 64 - 2),
        (AK_EXPR_INT, 0, 3, 2 ** 54 + 1), (AK_EXPR_INT, 0, 2 ** 63, 2 ** 127 - 2 ** 70), (AK_EXPR_INT, 0, 6, 0), (AK_EXPR_INT, 0, 5, 2 ** 127), (AK_EXPR_INT, 0, 3, 10)]
for _ in range(200):
    AVGS.append((AK_EXPR_INT, 0, max(1, int(RNG.integers(1, 2 ** 63)) >> int(RNG.integers(0, 62))), rand_value(int(RNG.integers(1, 128)))))
    AVGS.append((AK_EXPR_DEC, int(RNG.integers(0, 39)), max(1, int(RNG.integers(1, 2 ** 63)) >> int(RNG.integers(0, 62))), rand_value(int(RNG.integers(1, 126)))))


def row_text(row):
    return " ".join("%s=%s" % (c, "null" if v is None else (float(v).hex() if isinstance(v, float) else v)) for c, v in row.items())


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    d = tmp_path_factory.mktemp("agg_expr")
    exe, cases = str(d / "agg_expr_check"), str(d / "cases.txt")
    evals = dict(EDGES)
    evals.update(rand_evals())
    with open(cases, "w") as f:
        for name, (e, _, _, _) in PLANS.items():
            f.write("plan %s %d %s\n" % (name, SUM_EXPR, " ".join(XM.tokens(e))))
        for name, (text, _, _) in RAW.items():
            f.write("plan %s %s\n" % (name, text))
        for name, (e, _, _) in FOLDS.items():
            f.write("plan %s %d %s\n" % (name, SUM_EXPR, " ".join(XM.tokens(e))))
        for name, (e, _, row) in evals.items():
            f.write("eval %s %s | %s\n" % (name, " ".join(XM.tokens(e)), row_text(row)))
        for k, (op, a, b) in enumerate(ARITH):
            f.write("arith a%d %s %d %d\n" % (k, op, a, b))
        for k, (kind, scale, count, total) in enumerate(AVGS):
            f.write("avg v%d %d %d %d 0 %d\n" % (k, kind, scale, count, total))
        f.write("avg f_avg %d 0 4 0 %s\navg f_null %d 0 0 0 0\navg d_null %d 2 0 0 0\navg i_null %d 0 0 0 0\navg d_sticky %d 2 3 1 5\navg i_sticky %d 0 3 1 5\n"
                % (AK_SUM_F64, (10.5).hex(), AK_SUM_F64, AK_SUM_DEC, AK_SUM_INT, AK_EXPR_DEC, AK_EXPR_INT))
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "agg_expr_check.cpp")])
    run = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    got = {}
    for ln in run.stdout.splitlines():
        head, _, msg = ln.partition("\t")
        f = head.split()
        got[(f[0], f[1])] = (f[2:], msg)
    return got, evals


def test_class_table_scale_rule_slots_and_nodes(out):
    got, _ = out
    for name, (e, status, want, scale) in PLANS.items():
        f, msg = got[("plan", name)]
        assert int(f[0]) == status, (name, f, msg)
        if status == OK:
            assert (int(f[1]), int(f[2])) == (want, scale), (name, f)
            assert 1 <= int(f[4]) <= 4 and int(f[4]) == XM.slots(e), (name, f)
        else:
            assert want in msg, (name, msg)
    assert got[("plan", "balanced_8")][0][4] == "4" and got[("plan", "left_chain_16")][0][4] == "2" and got[("plan", "right_chain_16")][0][4] == "2"
    assert PLANS["nodes_31"][0].node_count() == 31 and PLANS["nodes_32"][0].node_count() == 32 and PLANS["nodes_33"][0].node_count() == 33


def test_malformed_trees(out):
    got, _ = out
    for name, (_, status, word) in RAW.items():
        f, msg = got[("plan", name)]
        assert int(f[0]) == status and word in msg, (name, f, msg)
    assert got[("plan", "avg_expr")][0][1:3] == [str(AK_EXPR_DEC), "4"]


def test_literal_folding(out):
    got, _ = out
    for name, (_, n_ops, slots) in FOLDS.items():
        f, msg = got[("plan", name)]
        assert (int(f[0]), int(f[3]), int(f[4])) == (OK, n_ops, slots), (name, f, msg)


def test_evaluator_against_python_ints(out):
    got, evals = out
    seen = {0: 0, 1: 0, 2: 0}
    for name, (e, cls, row) in evals.items():
        f, _ = got[("eval", name)]
        assert int(f[0]) == OK, (name, f)
        want = XM.eval_row(e, {"int": XM.INT, "dec": XM.DEC, "float": XM.FLOAT}[cls], row, SCALE)
        kind = 0 if want is None else 2 if want == XM.ROW_OVERFLOW else 1
        seen[kind] += 1
        assert int(f[1]) == kind, (name, f, want)
        if kind == 1:
            assert (float.fromhex(f[2]) == want) if cls == "float" else (int(f[2]) == want), (name, f, want)
    assert min(seen.values()) > 3, seen
    for name, fits in (("neg_2_64_times_2_63", 1), ("min_by_product", 1), ("max_plus_1_by_product", 2), ("p_2_64_times_2_63", 2), ("max_plus_1", 2), ("max_minus_1", 1),
                       ("min_minus_1", 2), ("min_plus_1", 1), ("neg_min", 2), ("neg_max", 1), ("sub_min", 2), ("rescale_38_one", 1), ("rescale_38_two", 2), ("null_gate", 0),
                       ("null_first", 0)):
        assert int(got[("eval", name)][0][1]) == fits, name
    assert int(got[("eval", "min_by_product")][0][2]) == I128_MIN and int(got[("eval", "rsub")][0][2]) == 5 - (49 + 5)
    assert float.fromhex(got[("eval", "float_no_fma")][0][2]) == 0.0          # the product rounds to 1.0 first; a fused multiply-add would give -2^-60


def test_checked_arithmetic(out):
    got, _ = out
    for k, (op, a, b) in enumerate(ARITH):
        want = a * b if op == "mul" else a + b if op == "add" else a - b if op == "sub" else -a if op == "neg" else a * 10 ** b
        f, _ = got[("arith", "a%d" % k)]
        assert int(f[0]) == int(I128_MIN <= want <= I128_MAX), (op, a, b, f)
        if int(f[0]):
            assert int(f[1]) == want, (op, a, b)


def test_avg_division(out):
    got, _ = out
    differs = 0
    for k, (kind, scale, count, total) in enumerate(AVGS):
        f, _ = got[("avg", "v%d" % k)]
        if kind in (AK_SUM_INT, AK_EXPR_INT):
            assert f[0] == str(KIND_F64) and f[1] == "0"
            assert int(f[2]) == int(not I128_MIN <= total <= I128_MAX), (k, f)
            if f[2] == "0":
                want = float(fractions.Fraction(total, count))
                assert float.fromhex(f[4]) == want == XM.avg_int(total, count), (k, total, count, f)
                differs += want != float(total) / count
        else:
            q, rs = XM.avg_decimal(total, count, scale)
            over = abs(total) >= T38 or abs(q) >= T38
            assert f[0] == str(KIND_DEC128) and f[1] == "0" and int(f[2]) == int(over) and int(f[3]) == rs == min(scale + 4, 38), (k, f)
            if not over:
                assert int(f[4]) == q, (k, kind, scale, count, total, f)
    assert differs > 10       # sums past 2^53: the correctly rounded quotient is not double(sum) / count
    assert got[("avg", "f_avg")][0][:3] == [str(KIND_F64), "0", "0"] and float.fromhex(got[("avg", "f_avg")][0][4]) == 10.5 / 4
    for name, kind in (("f_null", KIND_F64), ("d_null", KIND_DEC128), ("i_null", KIND_F64)):
        assert got[("avg", name)][0][:2] == [str(kind), "1"], name
    assert got[("avg", "d_sticky")][0][2] == "1" and got[("avg", "i_sticky")][0][2] == "1"
