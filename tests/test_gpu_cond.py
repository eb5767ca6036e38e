"""when / case / coalesce / nullif / abs on the GPU (orc_rust_amd.aggregate; the AX_CMP .. AX_PUSH_NULL ops of
device/agg_expr_eval.h inside compute_columns_cond_kernel, filter_expr_cond_kernel and the expression aggregates' *_cond_* kernels)
against tests/cond_model.py, row for row and exactly; doubles bit for bit.  The files, the columns and the shapes are those of
tests/test_gpu_div.py: 1 .. 2049 rows at batch size 1024 in one stripe, 3073 rows in four with a last stripe of one row; Byte, Short,
Int, Long, Date, Decimal at two scales, Float and Double columns; NULLs at word edges, a column without a PRESENT stream (dn, id) and
one that is all NULL (the NULL literal's branch).  Every test but the last two needs the new nodes."""
import decimal

import pyarrow as pa
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import agg_expr_model as AEM
import cond_model as M
import div_model as DM
import selection_model as SM
import test_gpu_div as D
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg, col
from orc_rust_amd.arrow_reader import concat_batches
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
from orc_rust_amd.top_k import SortKey

pytestmark = pytest.mark.gpu

SCHEMA, BATCH = D.SCHEMA, D.BATCH


def exprs_a():
    from orc_rust_amd.aggregate import abs_, case, coalesce, nullif, when
    L, Mc, p, q, i, h, t = (col(n) for n in ("L", "M", "p", "q", "i", "h", "t"))
    return {
        "bucket": case([(i < -2 ** 30, 0), (i < 2 ** 30, 1)], 2),              # a three-way bucket; NULL i: UNKNOWN twice, the last branch
        "cz": coalesce("ps", 0),                                               # COALESCE(x, 0)
        "nz": L / nullif(Mc, 0),                                               # a / NULLIF(b, 0): NULL, not an overflow, on a zero divisor
        "guard": when(h.ne(0), i // h, 0),                                     # the untaken branch divides by zero
        "gand": when(h.ne(0) & (i // h > 2), i % h, -1),                       # ... behind a FALSE AND
        "gor": when(h.eq(0) | (t // h < 0), 1, 0),                             # ... behind a TRUE OR
        "ovt": when(L > Mc, p * q, q),                                         # the taken branch overflows (p * q leaves 128 bits) on some rows only
        "ovc": when(p * q > 0, 1, when(P.is_null("p"), None, 0)),              # the condition overflows; a NULL literal's branch
        "pq": when(p < q, p, q),                                               # scales 2 and 4 aligned in CMP and in IF
        "ab": abs_(L - Mc) + abs(t),                                            # ABS; -2^63 - 2^63 fits 128 bits, not Int64
        "c2": coalesce(p, q, 7),                                               # both may be NULL: the third
    }


def exprs_b():
    from orc_rust_amd.aggregate import coalesce, when, year
    x, y, f, d = col("x"), col("y"), col("f"), col("d")
    return {
        "fw": when(x < y, x, y), "fn": when(x.ne(y), 1.0, 0.0), "fa": abs(x) + abs(f), "fc": coalesce(x / y, f, -1.0),
        # the f64 interpreter's AND / OR / NOT / IS_NULL, over doubles with NULLs, NaN and both infinities
        "f_and": when((x < y) & (f < 1.0), x, y), "f_or": when((x < y) | P.is_null("f"), x, -y), "f_not": when(~(x < y), 1.0, None),
        "f_isn": coalesce(when(~P.is_null("x") & ~(x >= y), None, x), f, 7.0),
        "yb": when(d > 0, year(d) % 100, None),                                # a date part and a division in a branch; an all-NULL else
        "an": when(P.gt("i", V.Int32(5)) & P.is_not_null("t"), col("i") - col("t"), col("g")),  # plain Predicate leaves
    }


def parts(exprs, most=8):
    """the expressions in lists of at most ORCGPU_COMPUTED_MAX: what one reader takes"""
    items = list(exprs.items())
    return [dict(items[k:k + most]) for k in range(0, len(items), most)]


class File(D.File):
    def model(self, e):
        vals, over = M.computed_column(e, SCHEMA, self.rows)
        if M.computed_type(e, SCHEMA)[0] == "float64":
            vals = [None if v is None else D.bits(v) for v in vals]
        return vals, over


def arrow_type_of(e):
    kind, s = M.computed_type(e, SCHEMA)
    return pa.int64() if kind == "int64" else pa.float64() if kind == "float64" else pa.decimal128(38, s)


def check_columns(f, table, reader, exprs):
    over = 0
    for k, e in exprs.items():
        want, o = f.model(e)
        over += o
        assert table.schema.field(k).type == arrow_type_of(e), k
        got = D.got_values(table, k)
        assert got == want, (k, [(n, a, b) for n, (a, b) in enumerate(zip(got, want)) if a != b][:5])
    assert reader.computed_overflow_rows() == over  # the model's count and not more: an untaken branch is not counted
    return over


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    return File(tmp_path_factory.mktemp("cond"), 3 * 1024 + 1, stripes=4, tag="big")


def test_the_nodes_are_new():
    """Fails without the feature: `from orc_rust_amd.aggregate import when` is an ImportError at the parent commit, and the C nodes
    21 .. 29 are ORCGPU_INVALID_ARGUMENT ("an unknown node") there."""
    from orc_rust_amd.aggregate import EXPR_IF, EXPR_NOT, when  # noqa: F401
    assert (EXPR_IF, EXPR_NOT) == (21, 29)


@pytest.mark.parametrize("n, stripes", [(1, 1), (63, 1), (64, 1), (65, 1), (1023, 1), (1024, 1), (1025, 1), (2049, 1), (3073, 4)])
def test_rows_against_the_model(tmp_path, n, stripes):
    f = File(tmp_path, n, stripes=stripes)
    for exprs in parts(exprs_a()) + parts(exprs_b()):
        reader = f.builder(list(exprs.items())).build()
        batches = list(reader)
        for b in batches:
            b.validate(full=True)
        table = concat_batches(batches)
        assert table.num_rows == n and table.schema.names == f.names + list(exprs)
        check_columns(f, table, reader, exprs)
    if n >= 1023:  # the data holds what the test is about, by the model's per-row outcomes
        ea = exprs_a()
        h0 = [r for r in f.rows if r["h"] == 0 and r["i"] is not None]
        assert h0 and all(M.computed_value(ea["guard"], SCHEMA, r) == (0, False) for r in h0)          # the untaken branch divides by zero
        assert all(M.computed_value(ea["gand"], SCHEMA, r) == (-1, False) for r in h0)
        assert all(M.computed_value(ea["gor"], SCHEMA, r) == (1, False) for r in f.rows if r["h"] == 0)
        assert DM.computed_column(col("i") // col("h"), SCHEMA, f.rows)[1] > 0                          # ... which overflows unguarded
        ovt = [M.computed_value(ea["ovt"], SCHEMA, r) for r in f.rows]
        assert (None, True) in ovt and any(not M.DM.fits(r["p"] * r["q"]) and o[1] is False and o[0] is not None
                                           for r, o in zip(f.rows, ovt) if r["p"] is not None and r["q"] is not None)  # untaken overflow: unseen
        assert (None, True) in [M.computed_value(ea["ovc"], SCHEMA, r) for r in f.rows]                 # an overflowed condition
        conds = {M.evaluate(ea["pq"].children[0], SCHEMA, r, False) for r in f.rows}
        assert {True, False, None} <= conds                                                             # TRUE, FALSE and UNKNOWN
        assert any(r["p"] is None and r["q"] is None for r in f.rows)                                   # both COALESCE operands NULL
        assert None in f.model(ea["nz"])[0] and f.model(ea["nz"])[1] < DM.computed_column(col("L") / col("M"), SCHEMA, f.rows)[1]
        assert arrow_type_of(ea["nz"]) == pa.decimal128(38, 6) and arrow_type_of(ea["pq"]) == pa.decimal128(38, 4) and arrow_type_of(ea["bucket"]) == pa.int64()


def test_no_present_stream_the_device_output_path_and_poison(big, monkeypatch):
    from orc_rust_amd.aggregate import coalesce, when
    exprs = {"wk": when(col("dn") % 7 < 3, col("id"), -col("id")), "cn": coalesce("dn", 0)}
    host = concat_batches(list(big.builder(exprs).with_projection(["id", "dn"]).build()))
    for k, e in exprs.items():
        want, over = big.model(e)
        assert D.got_values(host, k) == want and None not in want and over == 0, k
    over = 0
    for ea in parts(exprs_a()):
        reader = big.builder(ea).with_projection(["t", "h", "i", "L", "M", "p", "q", "ps"]).with_device_output().build()
        dev = concat_batches([b.to_pyarrow() for b in reader])
        assert reader.d2h_bytes() == 0
        over += check_columns(big, dev, reader, ea)
    assert over > 0
    monkeypatch.setenv("ORCGPU_POISON", "0xA5")  # a value or validity word left unwritten, or a NULL's value let through, shows
    for prefetch in (0, 2):
        for ea in parts(exprs_a()):
            reader = big.builder(ea, prefetch=prefetch).build()
            check_columns(big, concat_batches(list(reader)), reader, ea)


def kept_by(big, lhs, op, rhs, among):
    keep, over = [], 0
    for i in among:
        t, o = M.filter_leaf(lhs, op, rhs, big.rows[i], SCHEMA)
        over += 1 if o else 0
        if t is True:
            keep.append(i)
    return keep, over


def test_filter_leaves_under_a_selection_with_pruning_on_and_off(big):
    from orc_rust_amd.aggregate import coalesce, when
    sel = [(100, False), (30, True), (900, False), (70, True), (1200, False), (500, True), (273, False)]
    stripe_rows = [1024, 1024, 1024, 1]
    picked = [1024 * s + i for s, ranges in enumerate(SM.file_batches(sel, stripe_rows, BATCH)) for start, length in ranges for i in range(start, start + length)]
    ea = exprs_a()
    cases = [(ea["bucket"], "=", 1, False), (ea["guard"], ">", col("t"), False), (ea["ovt"], ">=", decimal.Decimal("0.5"), True),
             (coalesce("ps", 0), "<", col("ps") + 1, False), (exprs_b()["fw"], ">", 0.0, False), (exprs_b()["f_isn"], "<=", exprs_b()["f_or"], False), (col("i"), ">", when(col("h").ne(0), col("i") // col("h") * col("h"), None), False),
             (abs(col("L") - col("M")), "<", col("L") // col("M"), True)]
    outcomes = set()
    for lhs, op, rhs, overflows in cases:
        pred = P.compare(lhs, op, rhs)
        for use_sel in (False, True):
            among = picked if use_sel else list(range(big.n))
            want, over = kept_by(big, lhs, op, rhs, among)
            assert want, pred
            for prune in (True, False):
                b = big.builder().with_row_filter(pred, prune=prune).with_row_group_pruning(prune)
                if use_sel:
                    b = b.with_row_selection(sel)
                reader = b.build()
                batches = list(reader)
                got = concat_batches(batches).column("id").to_pylist() if batches else []
                assert got == want, (pred, use_sel, prune)
                assert reader.filter_overflow_rows() == over, (pred, use_sel, prune)
            assert (over > 0) == overflows, (pred, use_sel)
        outcomes |= {M.filter_leaf(lhs, op, rhs, r, SCHEMA) for r in big.rows}
    assert outcomes == {(True, False), (False, False), (None, False), (None, True)}


def dec(total, scale):
    return decimal.Decimal(total).scaleb(-scale, D.EXACT)


def specs():
    """three exact specs, then three of the FLOAT class whose values are 0, 0.25, 0.5, 1 and 2 -- their sums are exact in a double
    whatever the order of the reduction, so they are compared exactly -- over conditions with AND, OR, NOT and IS NULL on doubles
    that hold NULLs, NaN and both infinities"""
    from orc_rust_amd.aggregate import nullif, when
    x, y = col("x"), col("y")
    return [Agg.sum(when(col("i") > col("t"), col("i") - col("t"), 0)), Agg.avg(when(col("h").ne(0), col("ps") / col("h"), None)),
            Agg.sum(col("ps") / nullif(col("kn") - 1, 0)).where(P.gt("id", V.Int64(10))),
            Agg.sum(when((x < y) | P.is_null("y"), 1.0, 0.0)), Agg.sum(when(~(x < y) & P.is_not_null("f"), 0.5, None)),
            Agg.avg(when(~P.is_null("x") & ((x >= y) | (abs(x) > 1e300)), 2.0, 0.25))]


def model_aggs(big, idx):
    e = [s.expr for s in specs()]
    a = [v for v in (M.agg_row(e[0], SCHEMA, big.rows[i]) for i in idx) if v is not None]
    b = [v for v in (M.agg_row(e[1], SCHEMA, big.rows[i]) for i in idx) if v is not None]
    c = [v for v in (M.agg_row(e[2], SCHEMA, big.rows[i]) for i in idx if i > 10) if v is not None]
    assert AEM.ROW_OVERFLOW not in a + b + c
    avg = AEM.avg_decimal(sum(b), len(b), 6) if b else None
    f = [[v for v in (M.agg_row(e[k], SCHEMA, big.rows[i]) for i in idx) if v is not None] for k in (3, 4, 5)]
    assert all(v in (0.0, 0.25, 0.5, 1.0, 2.0) for vals in f for v in vals)
    return [sum(a) if a else None, dec(*avg) if avg else None, dec(sum(c), 6) if c else None,
            sum(f[0]) if f[0] else None, sum(f[1]) if f[1] else None, sum(f[2]) / len(f[2]) if f[2] else None]


def test_aggregates_plain_and_grouped(big):
    from orc_rust_amd.aggregate import when
    got = big.builder().aggregate(specs())
    want = model_aggs(big, range(big.n))
    assert got == want and None not in got and 0 < want[3] < big.n and want[4] > 0 and 0.25 < want[5] < 2.0
    groups = {}
    for i, r in enumerate(big.rows):
        groups.setdefault(r["g"], []).append(i)
    for limit in (None, 1024):
        res = big.builder().aggregate(specs(), group_by=["g"], max_groups=limit)
        assert [k[0] for k, _ in res] == list(groups)
        for (k, vals), idx in zip(res, groups.values()):
            assert vals == model_aggs(big, idx), (limit, k)
    # an overflow in the taken branch is AGG_OVERFLOW; the same division guarded is not
    with pytest.raises(OverflowError):
        big.builder().aggregate([Agg.sum(when(col("L") > 0, col("i") // col("h"), 0))])
    with pytest.raises(OverflowError):
        big.builder().aggregate([Agg.sum(when(col("p") * col("q") > 0, 1, 0))], group_by=["g"], max_groups=1024)


@pytest.mark.parametrize("limit", [None, 1024])
def test_group_by_a_computed_case_bucket_on_both_paths(big, limit):
    ea = exprs_a()
    exprs = {"bucket": ea["bucket"], "cz": ea["cz"]}
    vals = big.model(exprs["bucket"])[0]
    groups = {}
    for i in range(big.n):
        groups.setdefault(vals[i], []).append(i)
    assert set(groups) == {0, 1, 2}
    res = big.builder(exprs).aggregate([Agg.count_rows(), Agg.sum("cz"), Agg.sum(ea["guard"])], group_by=["bucket"], max_groups=limit)
    assert [k[0] for k, _ in res] == list(groups)
    for (k, got), idx in zip(res, groups.values()):
        cz = [big.rows[i]["ps"] or 0 for i in idx]
        gd = [v for v in (M.agg_row(ea["guard"], SCHEMA, big.rows[i]) for i in idx) if v is not None]
        assert got == [len(idx), dec(sum(cz), 2), sum(gd) if gd else None], (limit, k)


def test_top_k_by_abs_of_a_difference(big):
    e = abs(col("i") - col("t"))
    want, _ = big.model(e)
    got = big.builder({"ad": e}).top_k([SortKey("ad", descending=True, nulls_first=False), SortKey("id")], 40)
    exp = sorted(range(big.n), key=lambda i: (want[i] is None, -(want[i] or 0), i))[:40]
    assert got.column("id").to_pylist() == exp and D.got_values(got, "ad") == [want[i] for i in exp]


def test_collect_keys_of_a_case_bucket_used_in_in_set(big):
    e = exprs_a()["bucket"]
    want, _ = big.model(e)
    small = [i for i in range(1, big.n) if i % 97 == 0][:3]
    ks = big.builder({"bk": e}).with_row_filter(P.in_list("id", [V.Int64(i) for i in small]), prune=False).collect_keys("bk", max_keys=1 << 10)
    try:
        keys = {want[i] for i in small}
        assert len(ks) == len(keys)
        t = concat_batches(list(big.builder({"bk": e}).with_row_filter(P.in_set("bk", ks), prune=False).build()))
        assert t.column("id").to_pylist() == [i for i in range(big.n) if want[i] in keys]
    finally:
        ks.close()


def test_c_side_refusals(big):
    from orc_rust_amd.aggregate import EXPR_CMP, EXPR_IF, EXPR_NULL, Expr, when

    def refused(run, code, *fragments):
        with pytest.raises(capi.OrcGpuError) as e:
            run()
        assert e.value.code == code and all(f in str(e.value) for f in fragments), str(e.value)
    cond = Expr(EXPR_CMP, (col("i"), col("t")), cmp=2)
    refused(lambda: list(big.builder({"r": cond}).build()), 101, "CMP", "number is wanted", "computed column 'r'", "column 'i'")
    refused(lambda: list(big.builder({"r": Expr(EXPR_IF, (col("i"), col("t"), col("h")))}).build()), 101, "condition is wanted")
    refused(lambda: big.builder().aggregate([Agg.sum(col("i") + Expr(EXPR_NULL))]), 101, "NULL", "column 'i'")
    refused(lambda: list(big.builder({"r": when(col("i") > 0, col("x"), col("y"))}).build()), 6, "mixes the Float / Double column 'x'")
    refused(lambda: list(big.builder().with_row_filter(when(col("i") > 0, col("p"), col("x")) > 1, prune=False).build()), 6, "row filter:", "Float / Double")
    bad = Expr(EXPR_CMP, (col("i"), col("t")), cmp=9)
    refused(lambda: list(big.builder({"r": Expr(EXPR_IF, (bad, col("t"), col("h")))}).build()), 101, "names no comparison")
    deep = (col("i") + col("t")) * (col("h") + col("g"))
    refused(lambda: list(big.builder({"r": when(col("i") > 0, deep, deep)}).build()), 7, "more than ORCGPU_AGG_EXPR_MAX_DEPTH (4) operand slots")


def test_a_program_without_a_new_node_gives_what_it_gave(big):
    """the instantiations without the conditionals still run: the answers of tests/test_gpu_div.py's model"""
    exprs = {"pq": D.EXPRS_A["pq"], "rev": D.EXPRS_A["rev"], "sum": col("p") + col("q") * 2}
    reader = big.builder(exprs).build()
    table = concat_batches(list(reader))
    over = 0
    for k, e in exprs.items():
        want, o = DM.computed_column(e, SCHEMA, big.rows)
        over += o
        assert D.got_values(table, k) == want, k
    assert reader.computed_overflow_rows() == over
    want = [i for i in range(big.n) if DM.filter_leaf(col("i") % 1000, "<", col("t") * 3, big.rows[i], SCHEMA)[0] is True]
    assert concat_batches(list(big.builder().with_row_filter(col("i") % 1000 < col("t") * 3, prune=False).build())).column("id").to_pylist() == want
    assert big.builder().aggregate(D.SPECS) == D.model_aggs(big, range(big.n))
