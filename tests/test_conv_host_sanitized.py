"""The conversions of an expression under AddressSanitizer + UBSan on the CPU: tests/hostcheck/conv_check.cpp compiles the plan
compiler's pure include and device/agg_expr_eval.h -- the text liborcgpu.so is built from -- into a stand-alone program, run
directly; its lines are held to tests/conv_model.py.  No GPU."""
import os
import random
import shutil
import struct
import subprocess

import pytest

import agg_expr_model as AEM
import conv_model as M
import test_conv_model as TM
from orc_rust_amd import aggregate as A
from orc_rust_amd.aggregate import cast, ceil, col, decimal_, floor, lit, round_, trunc, when, year

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")

SCHEMA = {"a": "int", "b": "int", "i": "int", "d": "date", "p": ("dec", 2), "q": ("dec", 4), "w": ("dec", 10), "x": "float", "y": "float"}
INVALID, UNSUPPORTED, MISMATCHED = 101, 7, 6  # ORCGPU_INVALID_ARGUMENT, ORCGPU_UNSUPPORTED, ORCGPU_MISMATCHED_SCHEMA
AX = {"MARK": 14, "TO_F64": 25, "F64_TO_DEC": 26, "F64_TO_INT": 27, "RESCALE": 28, "FIT_I64": 29, "F64_ROUND": 30}


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def tokens(e):
    """an Expr as conv_check's tokens, in pre-order"""
    op = e.op
    if op == A.EXPR_COLUMN:
        out = ["c:" + e.column]
    elif op == A.EXPR_LITERAL:
        out = ["f:%x" % bits(e.value)] if e.value_type == A.PV_FLOAT64 else ["dec:%d:%d" % e.value] if e.value_type == A.PV_DECIMAL128 else ["i:%d" % e.value]
    elif op == A.EXPR_CMP:
        out = ["cmp:%d" % e.cmp]
    elif op == A.EXPR_CAST:
        out = ["cast:" + ("i" if e.value_type == A.PV_INT64 else "f" if e.value_type == A.PV_FLOAT64 else "d%d" % e.scale)]
    elif op == A.EXPR_ROUND:
        out = ["round:%d" % e.scale]
    elif op == A.EXPR_DATE_PART:
        out = ["year"]
    else:
        out = [{A.EXPR_ADD: "+", A.EXPR_SUB: "-", A.EXPR_MUL: "*", A.EXPR_NEG: "neg", A.EXPR_DIV: "/", A.EXPR_FLOOR_DIV: "//", A.EXPR_MOD: "%", A.EXPR_IF: "if",
                A.EXPR_COALESCE: "coalesce", A.EXPR_ABS: "abs", A.EXPR_NULL: "null", A.EXPR_IS_NULL: "isnull", A.EXPR_AND: "and", A.EXPR_OR: "or", A.EXPR_NOT: "not",
                A.EXPR_FLOOR: "floor", A.EXPR_CEIL: "ceil", A.EXPR_TRUNC: "trunc"}[op]]
    for c in e.children:
        out += tokens(c)
    return out


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("conv_check")
    exe = str(tmp / "conv_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "conv_check.cpp")])
    count = [0]

    def run(lines):
        count[0] += 1
        script = tmp / ("script%d.txt" % count[0])
        script.write_text("\n".join(lines) + "\n")
        return subprocess.run([exe, str(script)], check=True, capture_output=True, text=True).stdout.splitlines()
    return run


def test_every_case_of_the_model_test_through_the_real_functions(check):
    lines, want = [], []
    for s in TM.SCALES:
        for u in TM.UNSCALED:
            lines.append("f tof64 %d %d" % (u, s))
            want.append("f %x" % bits(M.to_f64(u, s)))
    for u in TM.UNSCALED:
        for k in (1, 2, 10, 22, 23, 38):
            for mode in range(4):
                lines.append("f rescale %d %d %d" % (u, k, mode))
                want.append("f %d" % M.rescale(u, k, mode))
    for x in TM.DOUBLES:
        for t in TM.TARGETS:
            lines.append("f todec %x %d" % (bits(x), t))
            r = M.f64_to_dec(x, t)
            want.append("f 0 0" if r is M.OVER else "f 1 %d" % r)
        lines.append("f toi64 %x" % bits(x))
        r = M.f64_to_i64(x)
        want.append("f 0 0" if r is M.OVER else "f 1 %d" % r)
        for mode in range(4):
            lines.append("f fround %x %d" % (bits(x), mode))
            want.append("f %x" % bits(M.f64_round(x, mode)))
    got = check(lines)
    assert len(got) == len(want)
    for line, g, w in zip(lines, got, want):
        assert g == w, line


def test_seeded_random_values_through_the_real_functions(check):
    rng = random.Random(20261021)
    lines, want = [], []
    for _ in range(3000):
        u = rng.choice((1, -1)) * rng.getrandbits(rng.choice((8, 40, 53, 54, 64, 100, 126)))
        u = max(-(10 ** 38 - 1), min(10 ** 38 - 1, u))
        s = rng.choice((0, 1, 2, 5, 10, 18, 22, 23, 30, 38))
        lines.append("f tof64 %d %d" % (u, s))
        want.append("f %x" % bits(M.to_f64(u, s)))
        k, mode = rng.randint(1, 38), rng.randrange(4)
        lines.append("f rescale %d %d %d" % (u, k, mode))
        want.append("f %d" % M.rescale(u, k, mode))
    for _ in range(3000):
        x = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0] if rng.random() < 0.3 else rng.choice((1, -1)) * rng.random() * 10.0 ** rng.randint(-30, 40)
        if rng.random() < 0.2:
            x = round(x * 2) / 2 if abs(x) < 1e15 else x  # ties
        t = rng.choice((0, 2, 9, 22, 23, 38))
        lines.append("f todec %x %d" % (bits(x), t))
        r = M.f64_to_dec(x, t)
        want.append("f 0 0" if r is M.OVER else "f 1 %d" % r)
        lines.append("f toi64 %x" % bits(x))
        r = M.f64_to_i64(x)
        want.append("f 0 0" if r is M.OVER else "f 1 %d" % r)
        mode = rng.randrange(4)
        lines.append("f fround %x %d" % (bits(x), mode))
        want.append("f %x" % bits(M.f64_round(x, mode)))
    got = check(lines)
    assert len(got) == len(want)
    for line, g, w in zip(lines, got, want):
        assert g == w, line


PROGRAMS = {
    "dec_times_dbl": cast("p", "float64") * col("x"),
    "dbl_to_dec_plus_dec": cast(col("x") * 100, decimal_(2)) + col("p"),
    "untaken_overflow": when(col("x") > 0, cast("x", "int64"), floor("p")),
    "year_of_cast": year(cast("x", "int64")),
    "long_as_double_by_3": cast("a", "float64") / 3,
    "wide_to_double": cast("w", "float64"),
    "wide_round_4": round_("w", 4),
    "wide_ceil": ceil("w"),
    "wide_trunc": trunc("w"),
    "wide_floor_mod": floor("w") % 7,
    "dec_to_int": cast("q", "int64"),
    "dec_down": cast("w", decimal_(2)),
    "dec_up": cast("p", decimal_(10)),
    "int_to_int": cast(col("a") * col("b"), "int64"),
    "dbl_round": round_("x") + floor("y") * ceil("x") - trunc("y"),
    "dbl_to_dec38": cast("x", decimal_(38)),
    "chain": cast(cast(cast("x", decimal_(4)), "float64") * 2, "int64"),
    "coalesce_cast": A.coalesce(cast("a", "float64"), col("x"), 1),
    "cmp_cast": when(cast("a", "float64") > col("x"), col("a"), cast("x", "int64")),
}


def _rows(rng, n):
    ints = [0, 1, -1, 2 ** 53 + 1, -(2 ** 53) - 1, 2 ** 63 - 1, -2 ** 63, 7, 1000003]
    decs = [0, 5, -5, 150, -150, 12345, -12345, 10 ** 38 - 1, -(10 ** 38 - 1), 2 ** 64 + 1, 5 * 10 ** 9, -5 * 10 ** 9, 15 * 10 ** 9]
    out = []
    for _ in range(n):
        row = {}
        for c in ("a", "b", "i"):
            row[c] = None if rng.random() < 0.1 else rng.choice(ints) if rng.random() < 0.5 else rng.randint(-10 ** 6, 10 ** 6)
        for c in ("p", "q", "w"):
            row[c] = None if rng.random() < 0.1 else rng.choice(decs) if rng.random() < 0.4 else rng.randint(-10 ** 14, 10 ** 14)
        for c in ("x", "y"):
            row[c] = None if rng.random() < 0.1 else rng.choice(TM.DOUBLES) if rng.random() < 0.5 else rng.uniform(-1e6, 1e6)
        out.append(row)
    return out


def test_programs_on_seeded_random_rows(check):
    rng = random.Random(7)
    rows = _rows(rng, 300)
    lines, want = [], []
    for name, e in sorted(PROGRAMS.items()):
        lines.append("prog %s %s" % (name, " ".join(tokens(e))))
        kind, _ = M.computed_type(e, SCHEMA)
        for row in rows:
            lines.append("row " + " ".join("%s=%s" % (c, "%x" % bits(v) if c in "xy" else "%d" % v) for c, v in sorted(row.items()) if v is not None))
            v, over = M.computed_value(e, SCHEMA, row)
            if v is None:
                want.append("row %s %d 0" % (name, 2 if over else 0))
            else:
                want.append("row %s 1 %s" % (name, "%x" % bits(v) if kind == M.CM.FLOAT64 else "%d" % v))
    got = check(lines)
    assert len(got) == len(want)
    for line, g, w in zip([x for x in lines if x.startswith("row")], got, want):
        assert g == w, line


def _plan(check, e):
    line = check(["plan x " + (" ".join(tokens(e)) if isinstance(e, A.Expr) else e)])[0]
    head, _, msg = line.partition("\t")
    f = head.split()
    return int(f[2]), f[3:], msg


def test_refusals_with_status_and_message(check):
    for e, status, words in (
            (col("p") + col("x"), MISMATCHED, ("mixes", "cast")),
            (cast("p", "float64") + col("p"), MISMATCHED, ("Float / Double", "cast")),
            (round_("x", 2), UNSUPPORTED, ("ROUND", "decimal")),
            (year(floor("x")), MISMATCHED, ("year()", "int64")),
            (floor("x") % 2, MISMATCHED, ("%", "int64")),
            (year(round_("p", 1)), MISMATCHED, ("year()",)),
            ("op:30:5:0 c:a", INVALID, ("CAST", "target")),
            ("op:30:8:39 c:a", INVALID, ("CAST", "scale")),
            ("op:30:8:-1 c:a", INVALID, ("CAST", "scale")),
            ("round:39 c:a", INVALID, ("ROUND", "digits")),
            ("round:-1 c:a", INVALID, ("ROUND", "digits")),
            ("floor", INVALID, ("FLOOR", "child")),
            ("cast:f", INVALID, ("CAST", "child")),
            ("floor cmp:0 c:a c:b", INVALID, ("CMP", "number is wanted")),
            ("op:35 c:a", INVALID, ("unknown node",))):
        rc, _, msg = _plan(check, e)
        assert rc == status, (e, rc, msg)
        for w in words:
            assert w in msg, (e, msg)


def _ops(fields):
    return [tuple(int(x) for x in f.split(":")) for f in fields[3:]]


def test_folding_and_the_ops_of_each_conversion(check):
    kinds = lambda e: [o[0] for o in _ops(_plan(check, e)[1])]
    body = lambda e: kinds(e)[1:-5]  # (behind the mark, in front of the tail)
    PUSH_INT, PUSH_DEC, PUSH_F64, PUSH_LIT, MUL, SCALE10 = 1, 2, 3, 4, 8, 10
    assert kinds(cast("a", "float64"))[0] == AX["MARK"]
    assert body(cast("a", "float64")) == [PUSH_INT, AX["TO_F64"]]
    assert body(cast("x", "float64")) == [PUSH_F64]                      # nothing happens, no op
    assert body(cast("p", decimal_(4))) == [PUSH_DEC, SCALE10]
    assert body(cast("q", decimal_(2))) == [PUSH_DEC, AX["RESCALE"]]
    assert body(cast("x", decimal_(2))) == [PUSH_F64, AX["F64_TO_DEC"]]
    assert body(cast("a", decimal_(0))) == [PUSH_INT] and _plan(check, cast("a", decimal_(0)))[1][:2] == ["1", "0"]  # the class alone changes: no op
    assert body(cast("a", decimal_(0)) + col("p")) == [PUSH_INT, SCALE10, PUSH_DEC, 5]
    assert body(cast("a", "int64")) == [PUSH_INT, AX["FIT_I64"]]
    assert body(cast("q", "int64")) == [PUSH_DEC, AX["RESCALE"], AX["FIT_I64"]]
    assert body(cast("x", "int64")) == [PUSH_F64, AX["F64_TO_INT"]]
    assert body(floor("a")) == [PUSH_INT] and body(round_("a", 3)) == [PUSH_INT] and body(round_("p", 2)) == [PUSH_DEC]
    assert body(floor("x")) == [PUSH_F64, AX["F64_ROUND"]] and body(ceil("q")) == [PUSH_DEC, AX["RESCALE"]]
    # the mode of a rescale travels in bits 8 .. 9 of `col`, beside k
    ops = _ops(_plan(check, ceil("q"))[1])
    assert ops[2][:2] == (AX["RESCALE"], 4 | (M.CEIL << 8)) and ops[2][2] == 10 ** 4
    # a conversion of a literal alone is folded ...
    for e, lo in ((col("x") * cast(3, "float64"), bits(3.0)), (col("x") * cast(lit(A.decimal.Decimal("1.25")), "float64"), bits(1.25)),
                  (col("x") * floor(lit(2.5)), bits(2.0)), (col("a") * cast(lit(2.9), "int64"), 2), (col("a") * cast(lit(-2.5), decimal_(0)), 2 ** 64 - 3),
                  (col("a") + trunc(lit(A.decimal.Decimal("-7.9"))), 2 ** 64 - 7), (col("p") + round_(lit(A.decimal.Decimal("0.125")), 2), 13)):
        ops = _ops(_plan(check, e)[1])
        assert [o[0] for o in ops[1:-5]] in ([PUSH_INT, PUSH_LIT, MUL], [PUSH_F64, PUSH_LIT, MUL], [PUSH_INT, PUSH_LIT, 5], [PUSH_DEC, PUSH_LIT, 5]), e
        assert ops[2][2] == lo, (e, ops)
    # ... unless it overflows: then it is left to the rows
    assert body(col("a") + cast(lit(1e30), "int64")) == [PUSH_INT, PUSH_LIT, AX["F64_TO_INT"], 5]
    assert body(col("a") + cast(lit(float("nan")), decimal_(2))) == [PUSH_INT, PUSH_LIT, AX["F64_TO_DEC"], SCALE10, 5] or \
        body(col("a") + cast(lit(float("nan")), decimal_(2))) == [PUSH_INT, SCALE10, PUSH_LIT, AX["F64_TO_DEC"], 5]
    got = check(["prog o " + " ".join(tokens(col("a") + cast(lit(1e30), "int64"))), "row a=1"])
    assert got == ["row o 2 0"]
    # the class and scale of the result are the root's
    for e in PROGRAMS.values():
        rc, f, msg = _plan(check, e)
        kind, scale = M.computed_type(e, SCHEMA)
        assert rc == 0 and (int(f[0]), int(f[1])) == ({M.CM.INT64: 0, M.CM.DEC128: 1, M.CM.FLOAT64: 2}[kind], scale), (e, f, msg)


# What the programs of expressions WITHOUT a conversion node were before there was one: `op:col:lo` per op, as tests/hostcheck/
# cond_check.cpp printed them at the commit before the conversions (class, scale, then the ops).
BEFORE = {
    "* c:p - i:1 c:q": "1 6 7 0:4:0 0:5:0 4:0:10000 2:5:0 6:0:0 2:4:0 8:0:0",
    "* * c:p - i:1 c:q + i:1 c:q": "1 10 11 0:4:0 0:5:0 4:0:10000 2:5:0 6:0:0 2:4:0 8:0:0 4:0:10000 2:5:0 5:0:0 8:0:0",
    "/ c:a c:b": "1 6 5 0:0:0 0:1:0 1:0:0 1:1:0 12:6:1000000",
    "/ c:p c:q": "1 6 5 0:4:0 0:5:0 2:4:0 2:5:0 12:8:100000000",
    "% + c:a i:7 c:i": "0 0 7 0:0:0 0:2:0 1:0:0 4:0:7 5:0:0 1:2:0 14:0:0",
    "+ * year c:d i:100 c:i": "0 0 8 0:3:0 0:2:0 1:3:0 11:0:0 4:0:100 8:0:0 1:2:0 5:0:0",
    "* c:x - f:3ff0000000000000 c:y": "2 0 7 0:6:0 0:7:0 4:0:4607182418800017408 3:7:0 6:0:0 3:6:0 8:0:0",
    "/ c:x c:y": "2 0 5 0:6:0 0:7:0 3:6:0 3:7:0 12:0:0",
    "if cmp:4 c:b i:0 / c:a c:b i:0": "1 6 9 14:0:0 1:1:1 4:0:0 16:4:0 1:0:1 1:1:1 12:6:1000000 4:0:0 21:0:0",
    "coalesce c:x abs c:y": "2 0 7 14:0:0 3:6:1 3:7:1 23:0:0 22:0:0 4:0:9221120237041090560 5:0:0",
    "neg - c:p c:a": "1 2 7 0:4:0 0:0:0 2:4:0 1:0:0 10:2:100 6:0:0 9:0:0",
}


def test_a_program_without_a_conversion_is_op_for_op_what_it_was(check):
    for text, before in BEFORE.items():
        rc, f, msg = _plan(check, text)
        assert rc == 0, (text, msg)
        now = f[:3] + [x.rsplit(":", 1)[0] for x in f[3:]]
        assert " ".join(now) == before, text
        assert all(x.endswith(":0") for x in f[3:]), text  # (`hi`: no flag anywhere)


def test_the_two_sides_of_a_filter_leaf_meet_like_operands(check):
    pair = lambda l, r: check(["pair x %s | %s" % (" ".join(tokens(l)), " ".join(tokens(A.Expr._wrap(r))))])[0].partition("\t")
    head, _, msg = pair(cast("a", "float64") * 2, col("x"))
    assert head.split()[2:] == ["0", "2", "0", "0", "1", "1"], (head, msg)  # (both sides are programs for the mixed interpreter)
    head, _, msg = pair(floor("w"), 3)
    assert head.split()[2:5] == ["0", "1", "0"], (head, msg)
    head, _, msg = pair(cast("x", decimal_(4)), col("p"))
    assert head.split()[2:6] == ["0", "1", "4", "2"], (head, msg)
    head, _, msg = pair(floor("w"), col("x"))
    assert head.split()[2] == str(MISMATCHED) and "cast" in msg
