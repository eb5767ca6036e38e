"""SUM / AVG over arithmetic expressions and AVG of plain columns on the GPU (orcgpu_result_aggregate_exprs,
orcgpu_result_aggregate_groups_exprs, orcgpu_reader_set_aggregate_exprs: device/agg_expr_eval.h, agg_expr_partial_kernel,
agg_group_expr_partial_kernel) against the model of tests/agg_expr_model.py.  Small files are written with pyarrow.orc (two stripes:
with this project's writer); the expected values come from the table that was written, never from a read of the file."""
import ctypes as C
import decimal
import math
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import agg_expr_model as XM
import agg_model as AM
import group_model as GM
import test_gpu_aggregate as TA
from orc_rust_amd import aggregate as A
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg, col, lit
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

pytestmark = pytest.mark.gpu

D = decimal.Decimal
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISMATCHED, UNSUPPORTED, INVALID = 6, 7, 101
SIZES = (1, 63, 64, 65, 257, 1000)      # one word of the keep mask and its edges, a second block, a batch with nulls
PRICE, DISC, TAX = col("p"), col("d"), col("t")
DISC_PRICE = PRICE * (1 - DISC)
CHARGE = PRICE * (1 - DISC) * (1 + TAX)
SPECS = [Agg.count_rows(), Agg.sum(DISC_PRICE), Agg.sum(CHARGE), Agg.sum("p"), Agg.avg("p"), Agg.avg("d"), Agg.avg("i"), Agg.avg("f"),
         Agg.sum(col("i") * col("j") - 3 * col("i")), Agg.sum(PRICE + col("w")), Agg.sum(-col("w") * 2 + D("0.5")), Agg.sum(col("f") * (1 - col("g")) + 0.25),
         Agg.avg(DISC_PRICE), Agg.avg(col("i") * col("j")), Agg.avg(col("f") * col("g")), Agg.sum_product("p", "d"), Agg.min("i"), Agg.max("f")]
NAMES = ["id", "p", "d", "t", "w", "i", "j", "f", "g", "flag", "half"]
_T, _F = {}, {}


def make_table(n, null_frac=None):
    if null_frac is None:
        null_frac = 0.33 if n == 1000 else 0.1 if n > 1 else 0.0
    key = (n, null_frac)
    if key in _T:
        return _T[key]
    rng = np.random.default_rng(100 + n)

    def nulls(values):
        return [None if m else v for v, m in zip(values, rng.random(n) < null_frac)]

    ids = np.arange(n)
    _T[key] = pa.table({
        "id": pa.array(ids.astype(np.int64)),
        "p": pa.array(nulls([D(int(x)).scaleb(-2) for x in rng.integers(-10 ** 9, 10 ** 13, n)]), pa.decimal128(15, 2)),
        "d": pa.array(nulls([D(int(x)).scaleb(-2) for x in rng.integers(0, 11, n)]), pa.decimal128(15, 2)),
        "t": pa.array(nulls([D(int(x)).scaleb(-2) for x in rng.integers(0, 9, n)]), pa.decimal128(15, 2)),
        "w": pa.array(nulls([D(int(x)).scaleb(-5) for x in rng.integers(-10 ** 11, 10 ** 11, n)]), pa.decimal128(12, 5)),
        "i": pa.array(nulls(rng.integers(-2 ** 62, 2 ** 62, n).tolist()), pa.int64()),
        "j": pa.array(nulls(rng.integers(-2 ** 31, 2 ** 31, n).tolist()), pa.int32()),
        "f": pa.array(nulls((rng.standard_normal(n) * 1e6).tolist()), pa.float64()),
        "g": pa.array(nulls(rng.random(n).astype(np.float32).tolist()), pa.float32()),
        "flag": pa.array([("A", "N", "R", None)[(x * 7) % 4] for x in ids], pa.string()),
        "half": pa.array((ids % 2).astype(np.int8), pa.int8()),
    })
    return _T[key]


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    capi.load()
    return tmp_path_factory.mktemp("aggregate_expr")


def write(tmpdir, table, name):
    if name not in _F:
        path = str(tmpdir / (name + ".orc"))
        orc.write_table(table, path, compression="uncompressed", stripe_size=64 << 20)
        _F[name] = path
    return _F[name]


def want_of(table, spec, keep):
    if spec.op in (A.SUM_EXPR, A.AVG, A.AVG_EXPR):
        return XM.aggregate_expr(table, spec, keep)
    return AM.aggregate_one(table, spec, keep)


def check(table, specs, got, keep, what):
    for s, g in zip(specs, got):
        w = want_of(table, s, keep)
        if isinstance(w, float) and XM.is_finite(w) and s.op in (A.SUM_EXPR, A.AVG, A.AVG_EXPR, A.SUM, A.SUM_PRODUCT):
            e = A.col(s.column) if s.op == A.AVG else s.expr
            if e is not None and s.op != A.SUM_EXPR and all(AM.column_values(table, x.column)[1] == "int" for x in XM.leaves(e) if x.op == A.EXPR_COLUMN):
                assert g == w, (what, s, g, w)       # an integer average is the correctly rounded quotient: exact
                continue
            terms = XM.float_terms(table, s, keep) if s.op != A.SUM and s.op != A.SUM_PRODUCT else AM.float_terms(table, s, keep)
            bound = AM.float_bound(terms) / (len(terms) if s.op in (A.AVG, A.AVG_EXPR) else 1)
            if s.op in (A.AVG, A.AVG_EXPR):
                bound += abs(w) * 2.0 ** -52     # the division rounds once more
            print(what, s, "got %r want %r bound %r" % (g, w, bound))
            assert isinstance(g, float) and abs(g - w) <= bound, (what, s, g, w, bound)
        else:
            assert AM.same(g, w), (what, s, g, w)


def drain_groups(reader, specs):
    try:
        raw = reader.aggregate(raw=True)
        return [(keys, [AM.OVERFLOW if v.overflow else A.value_of(v, s) for v, s in zip(vals, specs)]) for keys, vals in raw], reader.d2h_bytes()
    finally:
        reader.close()


def check_groups(table, specs, group_by, got, keep, what):
    want = GM.group_rows(table, group_by, keep, "ns")
    assert [tuple(GM.key_id(k) for k in keys) for keys, _ in got] == [tuple(GM.key_id(k) for k in keys) for keys, _ in want], what
    for (keys, vals), (_, mask) in zip(got, want):
        sub = table.filter(pa.array(mask))
        check(sub, specs, vals, np.ones(sub.num_rows, bool), (what, keys))


@pytest.mark.parametrize("n", SIZES)
def test_every_size_under_filter_selection_and_group_by(tmpdir, n):
    table = make_table(n)
    path = write(tmpdir, table, "t%d" % n)
    pred = P.and_([P.gte("id", V.Int64(n // 5)), P.gte("d", V.Decimal128(D("0.02")))])
    sel = [(max(1, n // 3), True), (max(1, n // 4), False), (n, True)]
    for name, p, s in (("all", None, None), ("filter", pred, None), ("selection", None, sel), ("both", pred, sel)):
        keep = AM.kept_mask(table, p, s, TA.BATCH)
        got, (seen, kept), d2h = TA.run(path, NAMES, SPECS, pred=p, selection=s)
        check(table, SPECS, got, keep, (n, name))
        assert d2h == 0 and kept == int(keep.sum()), (n, name, d2h, kept)
        for group_by in (["flag"], ["half", "flag"]):
            r = TA.builder(path, NAMES, pred=p, selection=s).aggregating_reader(SPECS, group_by=group_by)
            groups, d2h = drain_groups(r, SPECS)
            check_groups(table, SPECS, group_by, groups, keep, (n, name, group_by))
            assert d2h == 0
    # a mixed list gives, for the plain aggregates, exactly what the list without the expressions gives
    plain = [s for s in SPECS if s.expr is None and s.op != A.AVG]
    got_plain, _, _ = TA.run(path, NAMES, plain)
    got_all = dict(zip(map(id, SPECS), TA.run(path, NAMES, SPECS)[0]))
    for s, g in zip(plain, got_plain):
        assert (g is None and got_all[id(s)] is None) or (isinstance(g, float) and g.hex() == got_all[id(s)].hex()) or g == got_all[id(s)], s


def test_two_stripes_merge_on_the_host():
    table = make_table(1000)
    data, _ = TA.own_file(table, stripes=2)
    got, _, d2h = TA.run(data, NAMES, SPECS)
    check(table, SPECS, got, np.ones(1000, bool), "two stripes")
    assert d2h == 0
    r = TA.builder(data, NAMES, prefetch=2).aggregating_reader(SPECS, group_by=["flag", "half"])
    groups, d2h = drain_groups(r, SPECS)
    check_groups(table, SPECS, ["flag", "half"], groups, np.ones(1000, bool), "two stripes grouped")
    assert d2h == 0


def test_int_triple_product_overflows_in_exactly_one_row(tmpdir):
    n = 130
    a = np.full(n, 3, np.int64)
    b = np.full(n, -5, np.int64)
    a[0], b[0] = 2 ** 63 - 1, -2 ** 63          # the extremes: |a * b * a| < 2^189 but the first product fits, the second does not
    a[77], b[77] = -2 ** 63, 2 ** 63 - 1
    a[100], b[100] = 2 ** 62, 2 ** 62           # 2^186: the one row that leaves 128 bits ... with rows 0 and 77
    table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "a": pa.array(a), "b": pa.array(b)})
    path = write(tmpdir, table, "extremes")
    e = col("a") * col("b") * col("a")
    only = P.and_([P.ne("id", V.Int64(0)), P.ne("id", V.Int64(77))])        # rows 0 and 77 out: exactly one row overflows
    keep = AM.kept_mask(table, only)
    assert sum(XM.eval_row(e, XM.INT, {"a": int(x), "b": int(y)}, {}) == XM.ROW_OVERFLOW for x, y, k in zip(a, b, keep) if k) == 1
    specs = [Agg.sum(e), Agg.sum(col("a") * col("b")), Agg.count_rows()]
    got, _, _ = TA.run(path, ["id", "a", "b"], specs, pred=only)
    assert got[0] == AM.OVERFLOW and got[1] == XM.aggregate_expr(table, specs[1], keep) and got[2] == n - 2      # sticky; the others are untouched
    with pytest.raises(OverflowError) as err:
        TA.builder(path, ["id", "a", "b"], pred=only).aggregate(specs)
    assert "col('a')" in str(err.value)
    no_big = P.and_([only, P.ne("id", V.Int64(100))])
    got, _, _ = TA.run(path, ["id", "a", "b"], specs, pred=no_big)
    assert got[0] == XM.aggregate_expr(table, specs[0], AM.kept_mask(table, no_big)) == (n - 3) * -45
    # a * b alone fits at the extremes: -(2^63 - 1) * 2^63 twice
    got, _, _ = TA.run(path, ["id", "a", "b"], [specs[1]], pred=P.or_([P.eq("id", V.Int64(0)), P.eq("id", V.Int64(77))]))
    assert got == [2 * -(2 ** 63 - 1) * 2 ** 63]


def test_decimal_38_0_pair_that_sum_product_flags_and_the_minus_2_127_row(tmpdir):
    x = [D(2 ** 64), D(-2 ** 70), D(5), None]
    y = [D(2 ** 40), D(3), D(-(2 ** 80)), D(1)]
    m = [-2 ** 63, 2 ** 62, 2 ** 62, 0]             # m * 2^32 * 2^32: -2^127 balanced by two 2^126 rows
    table = pa.table({"x": pa.array(x, pa.decimal128(38, 0)), "y": pa.array(y, pa.decimal128(38, 0)), "m": pa.array(m, pa.int64()),
                      "k": pa.array([2 ** 32] * 3 + [0], pa.int64())})
    path = write(tmpdir, table, "dec38")
    specs = [Agg.sum_product("x", "y"), Agg.sum(col("x") * col("y")), Agg.sum(col("m") * col("k") * col("k")), Agg.avg(col("x") * col("y"))]
    got, _, _ = TA.run(path, ["x", "y", "m", "k"], specs)
    total = 2 ** 104 - 3 * 2 ** 70 - 5 * 2 ** 80
    assert got[0] == AM.OVERFLOW                     # an operand past 64 bits: what SUM_PRODUCT cannot do
    assert got[1] == D(total) and got[2] == 0       # exact; and -2^127 is a value like another
    q, rs = XM.avg_decimal(total, 3, 0)
    assert got[3] == D(q).scaleb(-rs, XM.EXACT) and rs == 4


def test_float_expression_is_deterministic_bit_for_bit(tmpdir):
    table = make_table(1000)
    path = write(tmpdir, table, "t1000")
    specs = [Agg.sum(col("f") * (1 - col("g")) + 0.25), Agg.avg(col("f") * col("g") - col("f"))]
    a, _, _ = TA.run(path, NAMES, specs)
    b, _, _ = TA.run(path, NAMES, specs)
    assert [x.hex() for x in a] == [x.hex() for x in b]
    check(table, specs, a, np.ones(1000, bool), "float")


def test_avg_over_no_row_and_over_nulls_and_an_all_null_group(tmpdir):
    n = 65
    ids = np.arange(n)
    table = pa.table({"id": pa.array(ids.astype(np.int64)), "i": pa.array([None] * n, pa.int64()), "f": pa.array([None] * n, pa.float64()),
                      "p": pa.array([None if x % 2 else D(int(x)).scaleb(-2) for x in ids], pa.decimal128(15, 2)), "q": pa.array([D(int(x)) for x in ids], pa.decimal128(15, 2)),
                      "half": pa.array((ids % 2).astype(np.int8), pa.int8())})
    path = write(tmpdir, table, "nulls")
    names = table.column_names
    specs = [Agg.avg("i"), Agg.avg("f"), Agg.avg("p"), Agg.avg(col("p") * col("q")), Agg.sum(col("p") * col("q")), Agg.sum(col("i") + 1), Agg.avg("q"), Agg.count_rows()]
    got, _, _ = TA.run(path, names, specs)
    check(table, specs, got, np.ones(n, bool), "nulls")
    assert got[0] is None and got[1] is None and got[5] is None and got[2] is not None
    got, _, _ = TA.run(path, names, specs, pred=P.lt("id", V.Int64(0)))                # no row at all
    assert got == [None] * 7 + [0]
    r = TA.builder(path, names).aggregating_reader(specs, group_by=["half"])            # the group half = 1: p is NULL in every row
    groups, _ = drain_groups(r, specs)
    check_groups(table, specs, ["half"], groups, np.ones(n, bool), "all-null group")
    assert groups[1][0] == (1,) and groups[1][1][2:5] == [None, None, None] and groups[1][1][6] is not None


def refused(b, specs, code, *words, **kw):
    r = b.aggregating_reader(specs, **kw)
    with pytest.raises(capi.OrcGpuError) as e:
        r.aggregate()
    assert e.value.code == code and all(w in str(e.value) for w in words), (specs, code, words, str(e.value))
    r.close()


def test_every_refusal(tmpdir):
    path = TA.pyarrow_file(tmpdir, 1025, 0.3)
    cols = TA.ALL_COLS
    for e, code, word in ((col("f64") + col("i64"), MISMATCHED, "'i64'"), (col("dec") * col("f32"), MISMATCHED, "'dec'"), (col("i64") * 0.5, MISMATCHED, "'i64'"),
                          (col("dec") + 0.5, MISMATCHED, "'dec'"), (col("f64") + D("0.5"), MISMATCHED, "'f64'"), (col("date") + 1, MISMATCHED, "'date'"),
                          (col("b") * 2, MISMATCHED, "'b'"), (col("ts") - 1, MISMATCHED, "'ts'"), (col("i64") + col("s"), MISMATCHED, "'s'"),
                          (col("i64") + col("nope"), INVALID, "'nope'"), (lit(1) + lit(2), INVALID, "no column"), (col("f64") + (2 ** 53 + 1), INVALID, "'f64'")):
        for ctor in (Agg.sum, Agg.avg):
            refused(TA.builder(path, cols), [ctor(e)], code, word)
    refused(TA.builder(path, ["id", "g"]), [Agg.sum(col("i64") + 1)], INVALID, "'i64'")                # not projected
    refused(TA.builder(path, cols).with_dictionary_columns(["s"]), [Agg.sum(col("s") + 1)], UNSUPPORTED, "'s'")
    sch = pa.schema([("id", pa.int64()), ("ts", pa.decimal128(38, 9))])
    refused(TA.builder(path, ["id", "ts"]).with_schema(sch), [Agg.sum(col("ts") + 1)], UNSUPPORTED, "'ts'")
    for name in ("s", "date", "b", "ts"):
        refused(TA.builder(path, cols), [Agg.avg(name)], MISMATCHED, "'%s'" % name)
    refused(TA.builder(path, cols), [Agg.avg("i64"), Agg.sum(col("i64") + col("s"))], MISMATCHED, "'s'", group_by=["g"])
    # the scale rule, the operand slots and the node count
    st = pa.table({"d20": pa.array([D(1).scaleb(-20)], pa.decimal128(38, 20)), "d19": pa.array([D(1).scaleb(-19)], pa.decimal128(38, 19)), "i": pa.array([2], pa.int64())})
    data, _ = TA.own_file(st)
    refused(TA.builder(data, st.column_names), [Agg.sum(col("i") + col("d20") * col("d19"))], UNSUPPORTED, "'i'", "38")
    assert TA.run(data, st.column_names, [Agg.sum(col("d19") * col("d19") - col("d20"))])[0] == [D(1 - 10 ** 18).scaleb(-38, XM.EXACT)]      # scale 38: accepted
    assert TA.run(data, st.column_names, [Agg.sum(col("d19") * col("d19") + col("i"))])[0] == [AM.OVERFLOW]      # 2 at scale 38 is 2 * 10^38: the rescale leaves 128 bits

    def balanced(k):
        return col("i") if k == 1 else balanced(k // 2) + balanced(k // 2)

    refused(TA.builder(data, st.column_names), [Agg.sum(balanced(16))], UNSUPPORTED, "operand slots")
    assert TA.run(data, st.column_names, [Agg.sum(balanced(8))])[0] == [16]
    chain = col("i")
    for _ in range(16):
        chain = chain - col("i")
    refused(TA.builder(data, st.column_names), [Agg.sum(chain)], INVALID, "32")


def test_malformed_trees_and_the_old_entry_points_through_the_c_abi():
    c = TA.ctx()
    res, table = TA.stripe_result(257, 100)
    names = (C.c_char_p * 2)(b"id", b"v")
    out = (A.AggValue * 2)()

    def call(specs, exprs):
        arr = (A.AggSpec * len(specs))(*specs)
        if exprs is None:
            return c.L.orcgpu_result_aggregate(c.h, res.h, None, 0, names, 2, arr, len(arr), out)
        return c.L.orcgpu_result_aggregate_exprs(c.h, res.h, None, 0, names, 2, arr, (A.AggExpr * len(exprs))(*exprs), len(arr), out)

    def expr(*nodes):
        arr = (A.AggExprNode * max(1, len(nodes)))(*nodes)
        keep.append(arr)
        return A.AggExpr(arr, len(nodes))

    keep = []
    v, one = A.AggExprNode(op=A.EXPR_COLUMN, column=b"v"), A.AggExprNode(op=A.EXPR_LITERAL, value_type=A.PV_INT64, i=1)
    add = A.AggExprNode(op=A.EXPR_ADD)
    for op in (A.SUM_EXPR, A.AVG_EXPR):
        assert call([A.AggSpec(op, b"v", None)], None) == INVALID                                     # the old entry point: no expression
        assert call([A.AggSpec(op, None, None)], [A.AggExpr(None, 0)]) == INVALID
        assert call([A.AggSpec(op, None, None)], [expr(add, v)]) == INVALID                            # an operand short
        assert call([A.AggSpec(op, None, None)], [expr(add, v, one, one)]) == INVALID                  # a node left over
        assert call([A.AggSpec(op, None, None)], [expr(add, v, A.AggExprNode(op=77))]) == INVALID
        assert call([A.AggSpec(op, None, None)], [expr(add, v, A.AggExprNode(op=A.EXPR_LITERAL, value_type=0, i=1))]) == INVALID      # a Boolean literal
        assert call([A.AggSpec(op, None, None)], [expr(add, v, A.AggExprNode(op=A.EXPR_LITERAL, value_type=A.PV_DECIMAL128, s=b"x" * 15, s_len=15, i=2))]) == INVALID
    assert call([A.AggSpec(9, b"v", None)], [A.AggExpr(None, 0)]) == INVALID                           # op 9 stays unknown
    assert call([A.AggSpec(A.SUM, b"v", None), A.AggSpec(A.SUM_EXPR, None, None)], [A.AggExpr(None, 0), expr(add, v, one)]) == 0
    want = AM.aggregate(table, [Agg.sum("v")])[0]
    assert A.value_of(out[0], None) == want and A.value_of(out[1], None) == want + AM.aggregate(table, [Agg.count("v")])[0]
    # the bindings, on a decoded result: plain, filtered and grouped
    specs = [Agg.sum(col("v") * col("id") + 1), Agg.avg("v"), Agg.avg(col("v") * 2), Agg.sum_product("v", "id")]
    pred = P.gt("v", V.Int64(10))
    for p in (None, pred):
        keepm = AM.kept_mask(table, p)
        check(table, specs, c.result_aggregate(res, specs, ["id", "v"], p), keepm, "result")
    groups = c.result_aggregate_groups(res, specs, ["v"], ["id", "v"], pred)
    check_groups(table, specs, ["v"], groups, AM.kept_mask(table, pred), "result groups")
    res.free()


CHILD = r'''
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
import test_gpu_aggregate_expr as T
from orc_rust_amd import capi
capi.load()
table = T.make_table(1000)
data, _ = T.TA.own_file(table, stripes=2)
for _ in range(2):      # (the second call reuses the workspace: what POISON is about)
    got = T.TA.builder(data, T.NAMES).aggregate(T.SPECS, group_by=["flag", "half"])
print("GROUPS", repr([(k, [v.hex() if isinstance(v, float) else v for v in vals]) for k, vals in got]))
'''


def test_poison_does_not_change_the_grouped_answer():
    lines = []
    for extra in ({}, {"ORCGPU_POISON": "0xA5"}):
        env = {k: v for k, v in os.environ.items() if not k.startswith("ORCGPU_")}
        env.update(extra)
        p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-3000:]      # (a child that faults fails here: no further child is started)
        lines.append([ln for ln in p.stdout.decode().splitlines() if ln.startswith("GROUPS")][-1])
    assert lines[0] == lines[1] and "Decimal" in lines[0]
