"""The row filter's expression leaf (Predicate.compare: lhs OP rhs) through the plan compiler under AddressSanitizer + UBSan on
the CPU: tests/hostcheck/filter_plan_expr_check.cpp compiles orc_rust_amd/csrc/orcgpu_filter_plan.inc -- the text liborcgpu.so is
built from, with orcgpu_agg_expr.inc, device/agg_expr_eval.h and device/filter_expr_eval.h behind it -- into a stand-alone
program that prints what became of every leaf and evaluates each compiled leaf on the rows given, with the evaluator the kernel
runs.  Here both are judged: the shapes by the rules of include/orcgpu.h, the rows by tests/filter_model_expr.py.  No GPU, nothing
loaded into Python."""
import os
import struct
import subprocess
from decimal import Decimal

import pytest

import filter_model_expr as M
from orc_rust_amd import aggregate as A
from orc_rust_amd.aggregate import col, lit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, MISMATCHED, UNSUPPORTED, INVALID = 0, 6, 7, 101
FOP_CMP_INT, FOP_CMP_FLOAT, FOP_CMP_DEC128, FOP_TRUE, FOP_FALSE, FOP_OR, FOP_AND, FOP_LIKE, FOP_IN, FOP_CMP_EXPR = 0, 1, 4, 8, 9, 11, 10, 13, 14, 15
EQ, NE, LT, LE, GT, GE = range(6)
OPS = ("=", "!=", "<", "<=", ">", ">=")
FXC_INT, FXC_DEC, FXC_FLOAT = 0, 1, 2
NAN, INF = float("nan"), float("inf")
SCHEMA = {"i8": "int", "i32": "int", "i64": "int", "j64": "int", "k64": "int", "d": "int", "e": "int", "f32": "float", "f64": "float", "g64": "float",
          "p": ("dec", 2), "q": ("dec", 7), "w": ("dec", 0), "v": ("dec", 0), "z": ("dec", 20)}
N_FLAT, N_ALL = 22, 23


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def tokens(e):
    if e.op == A.EXPR_COLUMN:
        return ["c:" + e.column]
    if e.op == A.EXPR_LITERAL:
        if e.value_type == A.PV_DECIMAL128:
            return ["d:%d:%d" % e.value]
        return ["f:%x" % bits(e.value)] if e.value_type == A.PV_FLOAT64 else ["i:%d" % e.value]
    out = [{A.EXPR_ADD: "+", A.EXPR_SUB: "-", A.EXPR_MUL: "*", A.EXPR_NEG: "neg"}[e.op]]
    for c in e.children:
        out += tokens(c)
    return out


def balanced(leaves):
    return leaves[0] if len(leaves) == 1 else balanced(leaves[:len(leaves) // 2]) + balanced(leaves[len(leaves) // 2:])


def chain(n_leaves):
    e = col("i64")
    for _ in range(n_leaves - 1):
        e = e + col("i64")
    return e


BIG = 10 ** 37
INT_ROWS = [dict(i8=1, i32=-7, i64=2 ** 63 - 1, j64=2 ** 63 - 1, k64=2 ** 63 - 1), dict(i8=-128, i32=5, i64=-2 ** 63, j64=3, k64=-1), dict(i8=None, i32=5, i64=1, j64=2, k64=3),
            dict(i8=0, i32=0, i64=0, j64=None, k64=0), dict(i8=5, i32=5, i64=5, j64=5, k64=25)]
DATE_ROWS = [dict(d=100, e=131), dict(d=100, e=130), dict(d=-5, e=-5), dict(d=None, e=1), dict(d=7, e=None), dict(d=2 ** 31 - 1, e=-2 ** 31)]
DEC_ROWS = [dict(p=150, q=15000000, w=BIG, v=BIG, z=5, i64=2), dict(p=-1, q=1, w=-BIG, v=3, z=-5, i64=-2), dict(p=None, q=1, w=1, v=1, z=1, i64=1),
            dict(p=0, q=0, w=0, v=0, z=0, i64=0), dict(p=10 ** 12 - 1, q=-(10 ** 20 - 1), w=10 ** 38 - 1, v=-(10 ** 38 - 1), z=10 ** 38 - 1, i64=2 ** 63 - 1),
            dict(p=5, q=None, w=BIG, v=BIG, z=None, i64=None), dict(p=199, q=19900001, w=17, v=-17, z=17 * 10 ** 20, i64=17)]
F32 = struct.unpack("<f", struct.pack("<f", 0.1))[0]
FLT_ROWS = [dict(f32=F32, f64=0.1, g64=0.2), dict(f32=0.0, f64=-0.0, g64=0.0), dict(f32=NAN, f64=1.0, g64=NAN), dict(f32=INF, f64=-INF, g64=INF), dict(f32=None, f64=1.0, g64=2.0),
            dict(f32=1.5, f64=1e308, g64=10.0), dict(f32=-1.0, f64=None, g64=None), dict(f32=2.0, f64=2.0, g64=4.0)]

# name -> (lhs, op, rhs, rows): every one compiles; its rows are judged by the model
EVAL = {}
for _k, _op in enumerate(OPS):
    EVAL["int_cols_%d" % _k] = (col("i64"), _op, col("j64"), INT_ROWS)
    EVAL["int_mixed_width_%d" % _k] = (col("i8") + col("i32"), _op, col("j64") - 1, INT_ROWS)
    EVAL["dec_scales_%d" % _k] = (col("p"), _op, col("q"), DEC_ROWS)
    EVAL["dec_final_rescale_%d" % _k] = (col("w"), _op, col("z"), DEC_ROWS)
    EVAL["dec_final_rescale_mirrored_%d" % _k] = (col("z"), _op, col("v"), DEC_ROWS)
    EVAL["flt_cols_%d" % _k] = (col("f64"), _op, col("g64"), FLT_ROWS)
    EVAL["flt_f32_%d" % _k] = (col("f32"), _op, col("f64"), FLT_ROWS)
EVAL.update({
    "int_sum_eq": (col("i64") * col("j64"), "=", col("k64"), INT_ROWS),
    "int_triple_product_overflows": (col("i64") * col("j64") * col("k64"), ">", col("i8"), INT_ROWS),
    "int_neg": (-col("i64"), "<", col("j64"), INT_ROWS),
    "int_literal_beyond_int64": (col("i64"), "<", lit(2 ** 63 - 1) + lit(5), INT_ROWS),
    "int_literal_folds_into_the_side": (col("i64") + col("j64"), ">=", lit(2) * lit(3) - 1, INT_ROWS),
    "date_vs_date": (col("d"), "<", col("e"), DATE_ROWS),
    "date_difference": (col("e") - col("d"), ">", lit(30), DATE_ROWS),
    "date_plus_int": (col("d") + col("i32"), "<=", col("e"), [dict(r, i32=k - 2) for k, r in enumerate(DATE_ROWS)]),
    "dec_q14": (col("p") * (1 - col("q")), ">", lit(Decimal("-0.75")), DEC_ROWS),
    "dec_int_column_beside": (col("p") * 2, "=", col("i64") + 1, DEC_ROWS),
    "dec_int_literal_beside": (col("i64"), "<", lit(Decimal("1.5")), DEC_ROWS),
    "dec_inner_overflow_product": (col("w") * col("v"), ">", lit(0), DEC_ROWS),
    "dec_inner_overflow_scale_up": (col("w") + col("z"), ">", col("p"), DEC_ROWS),
    "dec_inner_overflow_on_the_right": (col("p"), "<", col("v") * col("w"), DEC_ROWS),
    "dec_scale_38": (col("z") * col("q") * col("q"), "!=", col("p"), DEC_ROWS),  # 20 + 7 + 7 = 34; against scale 2
    "flt_q": (col("f64") * (1 - col("g64")), ">", lit(0.05), FLT_ROWS),
    "flt_int_literal": (col("f64") + 1, ">=", col("g64") * 2, FLT_ROWS),
    "flt_inf_minus_inf": (col("f32") - col("g64"), "=", lit(0.0), FLT_ROWS),
    # simple forms: a bare column against a side that folds to a literal
    "simple_int": (col("i64"), "<", lit(2) + lit(3), INT_ROWS),
    "simple_int_mirrored": (lit(5), "<", col("i64"), INT_ROWS),
    "simple_int_mirrored_le": (lit(10) - 5, "<=", col("i64"), INT_ROWS),
    "simple_int_eq_mirrored": (lit(5), "=", col("i32"), INT_ROWS),
    "simple_date": (col("d"), ">=", lit(100), DATE_ROWS),
    "simple_float": (col("f64"), ">", lit(0.05) * lit(2.0), FLT_ROWS),
    "simple_float_mirrored": (lit(0.1), ">=", col("f32"), FLT_ROWS),
    "simple_float_int_literal": (col("g64"), "=", lit(4), FLT_ROWS),
    "simple_dec": (col("p"), "<=", lit(Decimal("1.5")), DEC_ROWS),
    "simple_dec_off_scale": (col("p"), "<", lit(Decimal("1.505")), DEC_ROWS),
    "simple_dec_mirrored": (lit(Decimal("1.99")) + lit(Decimal("0.0000001")), ">", col("q"), DEC_ROWS),
    "simple_dec_int_literal": (col("z"), ">", lit(17) - lit(1), DEC_ROWS),
    "dec_literal_past_10_38_stays_general": (col("w"), "<", lit(Decimal(10 ** 37)) * lit(100), DEC_ROWS),
    # two literal sides
    "lits_true": (lit(2) * lit(3), "=", lit(6), INT_ROWS[:2]),
    "lits_false": (lit(Decimal("1.50")), "<", lit(Decimal("1.5")), DEC_ROWS[:2]),
    "lits_dec_vs_int": (lit(Decimal("1.50")), ">", lit(1), DEC_ROWS[:2]),
    "lits_float_nan": (lit(NAN), "!=", lit(NAN), FLT_ROWS[:2]),
    "lits_float_nan_eq": (lit(NAN), "=", lit(1), FLT_ROWS[:2]),
})

# name -> (lhs, op, rhs, status, the column the message must name or None, columns of the projection)
REFUSED = {
    "float_beside_int": (col("f64"), "<", col("i64"), MISMATCHED, "f64", N_FLAT),
    "float_beside_dec_other_side": (col("p") + 1, "<", col("g64"), MISMATCHED, "g64", N_FLAT),
    "float_literal_beside_int": (col("i64"), "<", lit(1.5), MISMATCHED, "i64", N_FLAT),
    "dec_literal_beside_float": (col("f64"), "<", lit(Decimal("1.5")), MISMATCHED, "f64", N_FLAT),
    "float_literal_beside_dec_literal": (lit(1.5), "<", lit(Decimal("1.5")), MISMATCHED, None, N_FLAT),
    "scale_39": (col("z") * col("z"), ">", col("p"), UNSUPPORTED, "z", N_FLAT),
    "scale_39_on_the_right": (col("p"), ">", col("z") * col("q") * col("q") * col("q"), UNSUPPORTED, "p", N_FLAT),
    "nodes_33": (chain(17), ">", col("j64"), INVALID, None, N_FLAT),
    "nodes_33_on_the_right": (col("j64"), ">", chain(17), INVALID, None, N_FLAT),
    "balanced_16": (balanced([col("i64")] * 16), ">", col("j64"), UNSUPPORTED, "i64", N_FLAT),
    "boolean": (col("b"), "=", lit(1), UNSUPPORTED, "b", N_FLAT),
    "string": (col("i64"), "<", col("s"), UNSUPPORTED, "s", N_FLAT),
    "varchar": (col("vc"), "<", col("s"), UNSUPPORTED, "vc", N_FLAT),
    "char": (col("ch") + 1, "<", lit(1), UNSUPPORTED, "ch", N_FLAT),
    "binary": (lit(1), "<", col("bin"), UNSUPPORTED, "bin", N_FLAT),
    "timestamp": (col("ts"), "<", col("tsi"), UNSUPPORTED, "ts", N_FLAT),
    "timestamp_instant": (col("i64"), "<", col("tsi"), UNSUPPORTED, "tsi", N_FLAT),
    "nested_in_the_projection": (col("i64"), "<", col("j64"), UNSUPPORTED, "st", N_ALL),
    "no_such_column": (col("i64"), "<", col("nope"), INVALID, "nope", N_FLAT),
    "int_literal_inexact_as_double": (col("f64"), "<", lit(2 ** 53 + 1), INVALID, "f64", N_FLAT),
}


def value_token(name, v):
    if v is None:
        return "%s=N" % name
    return "%s=x%x" % (name, bits(v)) if SCHEMA[name] == "float" else "%s=%d" % (name, v)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("filter_plan_expr")
    exe, cases = str(d / "filter_plan_expr_check"), str(d / "cases.txt")
    with open(cases, "w") as f:
        for name, (lhs, op, rhs, rows) in EVAL.items():
            f.write(" ".join(["case", name, str(OPS.index(op)), "0", "-", "L"] + tokens(lhs) + ["R"] + tokens(rhs)) + "\n")
            for row in rows:
                f.write(" ".join(["row"] + [value_token(k, v) for k, v in row.items()]) + "\n")
        for name, (lhs, op, rhs, _, column, n_columns) in REFUSED.items():
            f.write(" ".join(["case", name, str(OPS.index(op)), str(n_columns), column or "-", "L"] + tokens(lhs) + ["R"] + tokens(rhs)) + "\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "filter_plan_expr_check.cpp")])
    out = subprocess.run([exe, cases], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    return [ln.split() for ln in out.stdout.splitlines()]


def case(lines, name):
    """(status, named) for a refusal, else a dict of what the first instruction holds"""
    ln = [x for x in lines if x[0] == "case" and x[1] == name]
    assert len(ln) == 1, name
    ln = ln[0]
    if int(ln[2]) != OK:
        return int(ln[2]), int(ln[3])
    keys = ("n_insn", "op", "cmp", "i", "lo", "fbits", "col", "n_expr", "n_planes")
    d = {k: int(v, 16) if k == "fbits" else int(v) for k, v in zip(keys, ln[3:12])}
    d.update({k: v for k, v in (x.split("=") for x in ln[12:])})
    return d


def test_every_compiled_leaf_agrees_with_the_model_on_every_row(lines):
    n_rows = n_over = 0
    for name, (lhs, op, rhs, rows) in EVAL.items():
        assert isinstance(case(lines, name), dict), name
        got = [ln[3] for ln in lines if ln[0] == "row" and ln[1] == name]
        want = []
        for row in rows:
            t, over = M.evaluate(lhs, op, rhs, row, SCHEMA)
            want.append("O" if over else "U" if t is None else "T" if t else "F")
        assert got == want, (name, got, want)
        n_rows += len(rows)
        n_over += want.count("O")
    assert n_rows > 300 and n_over >= 8
    # the cases mean what their names say
    assert "O" in [ln[3] for ln in lines if ln[0] == "row" and ln[1] == "dec_inner_overflow_product"]
    assert [ln[3] for ln in lines if ln[0] == "row" and ln[1] == "dec_final_rescale_4"][:2] == ["T", "F"]  # 10^37 > 5e-20; -10^37 > -5e-20 is false
    assert "O" not in [ln[3] for ln in lines if ln[0] == "row" and ln[1].startswith("dec_final_rescale")]


def test_the_classes_and_the_general_form(lines):
    c = case(lines, "int_cols_2")
    assert (c["n_insn"], c["op"], c["cmp"], c["i"], c["n_expr"], c["n_planes"], c["cls"], c["d"], c["aligned"]) == (1, FOP_CMP_EXPR, LT, 0, 1, 2, str(FXC_INT), "0", "1")
    assert c["ops"] == "2,2"  # a gate and a push on each side
    assert case(lines, "date_vs_date")["cls"] == str(FXC_INT) and case(lines, "date_plus_int")["cls"] == str(FXC_INT)
    c = case(lines, "dec_scales_0")
    assert (c["op"], c["cls"], c["d"]) == (FOP_CMP_EXPR, str(FXC_DEC), "5")  # q's scale 7 minus p's 2
    assert case(lines, "dec_final_rescale_0")["d"] == "20" and case(lines, "dec_final_rescale_mirrored_0")["d"] == "-20"
    assert case(lines, "dec_int_column_beside")["cls"] == str(FXC_DEC) and case(lines, "dec_int_literal_beside")["cls"] == str(FXC_DEC)
    assert case(lines, "flt_cols_0")["cls"] == str(FXC_FLOAT) and case(lines, "flt_int_literal")["cls"] == str(FXC_FLOAT)
    # literals fold inside a side: (2 * 3 - 1) is one push
    assert case(lines, "int_literal_folds_into_the_side")["ops"] == "5,1"
    assert case(lines, "int_literal_beyond_int64")["op"] == FOP_CMP_EXPR and case(lines, "dec_literal_past_10_38_stays_general")["op"] == FOP_CMP_EXPR


def test_simple_forms_become_the_comparison_they_equal(lines):
    def shape(name):
        c = case(lines, name)
        return c["n_insn"], c["op"], c["cmp"], c["i"], c["n_planes"]

    assert shape("simple_int") == (1, FOP_CMP_INT, LT, 5, 0)
    assert shape("simple_int_mirrored") == (1, FOP_CMP_INT, GT, 5, 0)  # 5 < x is x > 5
    assert shape("simple_int_mirrored_le") == (1, FOP_CMP_INT, GE, 5, 0)
    assert shape("simple_int_eq_mirrored") == (1, FOP_CMP_INT, EQ, 5, 0)
    assert shape("simple_date") == (1, FOP_CMP_INT, GE, 100, 0)
    c = case(lines, "simple_float")
    assert (c["op"], c["cmp"], c["fbits"], c["n_planes"]) == (FOP_CMP_FLOAT, GT, bits(0.05 * 2.0), 0)
    c = case(lines, "simple_float_mirrored")
    assert (c["op"], c["cmp"], c["fbits"]) == (FOP_CMP_FLOAT, LE, bits(0.1))
    c = case(lines, "simple_float_int_literal")
    assert (c["op"], c["cmp"], c["fbits"]) == (FOP_CMP_FLOAT, EQ, bits(4.0))
    c = case(lines, "simple_dec")
    assert (c["op"], c["cmp"], c["i"], c["lo"], c["n_planes"]) == (FOP_CMP_DEC128, LE, 0, 150, 0)  # 1.5 at the column's scale 2
    c = case(lines, "simple_dec_off_scale")
    assert (c["op"], c["cmp"], c["i"], c["lo"]) == (FOP_CMP_DEC128, LE, 0, 150)  # < 1.505 is <= 1.50
    c = case(lines, "simple_dec_mirrored")
    assert (c["op"], c["cmp"], c["i"], c["lo"]) == (FOP_CMP_DEC128, LT, 0, 19900001)
    c = case(lines, "simple_dec_int_literal")
    assert (c["op"], c["cmp"], c["i"], c["lo"]) == (FOP_CMP_DEC128, GT, (16 * 10 ** 20) >> 64, (16 * 10 ** 20) & (2 ** 64 - 1))
    for name, want in (("lits_true", FOP_TRUE), ("lits_false", FOP_FALSE), ("lits_dec_vs_int", FOP_TRUE), ("lits_float_nan", FOP_TRUE), ("lits_float_nan_eq", FOP_FALSE)):
        c = case(lines, name)
        assert (c["n_insn"], c["op"], c["n_planes"]) == (1, want, 0), name


def test_refusals_name_the_column(lines):
    for name, (_, _, _, status, column, _) in REFUSED.items():
        assert case(lines, name) == (status, 1 if column else 0), name


def test_malformed_node_lists_and_the_depth(lines):
    bad = {ln[1]: int(ln[2]) for ln in lines if ln[0] == "bad"}
    assert len(bad) == 19 and bad.pop("fine") == OK
    assert set(bad.values()) == {INVALID}, bad
    depth = {int(ln[1]): (int(ln[2]), int(ln[3])) for ln in lines if ln[0] == "depth"}
    assert depth[63] == (OK, 64) and depth[64][0] == INVALID


def parse_dump(ln):
    at = ln.index("|")
    prog = [tuple(int(x) for x in p.split(":")) for p in ln[1:at]]
    rest = ln[at + 1:]
    like = [int(x) for x in rest[rest.index("like") + 1:rest.index("in")]]
    in_ = [int(x) for x in rest[rest.index("in") + 1:rest.index("expr")]]
    expr = [int(x) for x in rest[rest.index("expr") + 1:rest.index("planes")]]
    return prog, like, in_, expr, int(rest[rest.index("planes") + 1]), int(rest[rest.index("leaves") + 1])


def test_planes_are_numbered_with_the_like_and_in_planes_and_survive_the_merge(lines):
    assert [ln for ln in lines if ln[0] == "five"][0][1] == "0"
    prog, like, in_, expr, n_planes, n_leaves = parse_dump([ln for ln in lines if ln[0] == "planes"][0])
    # LIKE -> plane 0; d < e -> planes 1, 2; IN (1, 2) -> plane 3; 5 >= i32 -> the comparison i32 <= 5; p + q = w -> planes 4, 5
    assert [(op, i, cmp_) for op, i, cmp_, _ in prog] == [(FOP_LIKE, 0, 4), (FOP_CMP_EXPR, 1, LT), (FOP_OR, 0, 0), (FOP_IN, 3, 0), (FOP_OR, 0, 0), (FOP_CMP_INT, 5, LE),
                                                         (FOP_OR, 0, 0), (FOP_CMP_EXPR, 4, EQ), (FOP_OR, 0, 0)]
    assert all(pad == 0 for op, _, _, pad in prog if op in (FOP_CMP_EXPR, FOP_IN))  # op tables and hash sets on 8-byte boundaries
    assert (like, in_, expr, n_planes, n_leaves) == ([0], [3], [1, 7], 6, 4)
    assert [ln[1:] for ln in lines if ln[0] == "blob"][:2] == [["1", "1", "1"], ["7", "1", "1"]]
    # a condition of its own: f64 * g64 != 1.0 -> planes 0, 1; LIKE -> plane 2
    assert [ln for ln in lines if ln[0] == "cond"][0][1] == "0"
    cprog, clike, cin, cexpr, cplanes, _ = parse_dump([ln for ln in lines if ln[0] == "cond_planes"][0])
    assert [(op, i) for op, i, _, _ in cprog] == [(FOP_CMP_EXPR, 0), (FOP_LIKE, 2), (FOP_AND, 0)] and (clike, cin, cexpr, cplanes) == ([1], [], [0], 3)
    # ... behind the row filter's program: instructions from 9 on, planes from 6 on, the leaf lists carried, the op tables still aligned
    assert [ln for ln in lines if ln[0] == "merged_first"][0][1] == "9"
    mprog, mlike, min_, mexpr, mplanes, mleaves = parse_dump([ln for ln in lines if ln[0] == "merged"][0])
    assert mprog[:9] == prog and [(op, i) for op, i, _, _ in mprog[9:]] == [(FOP_CMP_EXPR, 6), (FOP_LIKE, 8), (FOP_AND, 0)]
    assert all(pad == 0 for op, _, _, pad in mprog if op in (FOP_CMP_EXPR, FOP_IN))
    assert (mlike, min_, mexpr, mplanes, mleaves) == ([0, 10], [3], [1, 7, 9], 9, 6)
    assert [ln[1:] for ln in lines if ln[0] == "blob"][2:] == [["1", "1", "1"], ["7", "1", "1"], ["9", "1", "1"]]
    # the columns the three leaves read: gates as "any" (6), values by the kind they are loaded as
    reads = [ln for ln in lines if ln[0] == "reads"][0][1:]
    assert reads == ["d:6", "d:0", "e:6", "e:0", "p:6", "q:6", "p:5", "q:5", "w:6", "w:5", "f64:6", "g64:6", "f64:1", "g64:1"]
