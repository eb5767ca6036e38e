"""year / quarter / month / day / day_of_week / day_of_year of a Date on the GPU (orc_rust_amd.aggregate.year .. extract; the
AX_DATE_PART op of device/agg_expr_eval.h inside compute_columns_kernel, filter_expr_kernel and the expression aggregates' kernels)
against tests/date_part_model.py, row for row and exactly.  Files are written in the test with pyarrow, one stripe or four, a few
thousand rows at most.  Every test here needs the new functions: none passes without the feature."""
import datetime
import decimal

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import agg_expr_model as AEM
import date_part_model as M
import selection_model as SM
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg, col, day, day_of_week, day_of_year, extract, month, quarter, year
from orc_rust_amd.arrow_reader import ArrowReaderBuilder, concat_batches
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
from orc_rust_amd.top_k import SortKey

pytestmark = pytest.mark.gpu

BATCH = 1024
EPOCH = datetime.date(1970, 1, 1).toordinal()
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
SCHEMA = {"id": "int", "g": "int", "d": "date", "dn": "date", "ds": "date", "k": "int", "L": "int", "p": ("dec", 2)}
ARROW = {"id": pa.int64(), "g": pa.int32(), "d": pa.date32(), "dn": pa.date32(), "ds": pa.date32(), "k": pa.int32(), "L": pa.int64(), "p": pa.decimal128(12, 2)}


def days_of(y, m, d):
    return datetime.date(y, m, d).toordinal() - EPOCH


# the int32 ends, 1970-01-01 +- 1, the leap days of 1600 / 1900 (none: 28 February and 1 March) / 2000 and their neighbours
SPECIAL = [I32_MIN, I32_MAX, I32_MIN + 1, I32_MAX - 1, -1, 0, 1, days_of(1600, 2, 29), days_of(1600, 3, 1), days_of(1900, 2, 28), days_of(1900, 3, 1),
           days_of(2000, 2, 29), days_of(2000, 3, 1), days_of(2000, 12, 31), days_of(1999, 12, 31), days_of(1, 1, 1) - 366, days_of(1, 1, 1) - 367]
EXPRS = {
    "y": year("d"), "q": quarter("d"), "m": month("d"), "dd": day("d"), "w": day_of_week("d"), "n": day_of_year("d"),  # all six parts at once
    "yk": year(col("d") + col("k")) * 100 + month(col("d") + col("k")),  # an operand that leaves int32 at the ends
    "yL": extract("year", col("L")),                                       # a Long operand: beyond int32, and beyond what d + k reaches
}
_CTX = None


def ctx():
    global _CTX
    if _CTX is None:
        _CTX = capi.Context()
    return _CTX


def make_columns(n, seed=11):
    """name -> the model's values (ints; None: NULL).  NULLs at word edges; dn has none (no PRESENT stream)."""
    rng = np.random.default_rng(seed + n)

    def nulls(values, frac=0.15):
        out = [None if z else v for v, z in zip(values, rng.random(n) < frac)]
        for edge in (0, 63, 64, 127, 128, n - 1):
            if 0 <= edge < n:
                out[edge] = None if edge % 2 == 0 else values[edge]
        return out

    lo, hi = days_of(1, 1, 1) - 2 * 366, days_of(9999, 12, 31) + 366  # the years -1 .. 10000
    spread = [int(v) for v in rng.integers(lo, hi, n)]
    for at, v in zip(rng.permutation(n)[:len(SPECIAL)], SPECIAL):
        spread[int(at)] = v
    c = {"id": list(range(n)), "d": nulls(spread)}
    c["dn"] = [int(v) for v in rng.integers(lo, hi, n)]
    c["ds"] = nulls([int(v) for v in rng.integers(days_of(1992, 1, 1), days_of(1998, 12, 31), n)])  # TPC-H's seven years: few groups
    c["k"] = nulls([[0, 1, -1, 30, -365, 366][int(v)] for v in rng.integers(0, 6, n)], 0.1)
    pool = [I32_MAX, I32_MAX + 1, I32_MIN, I32_MIN - 1, 2 ** 40, -2 ** 40, 2 ** 63 - 1, -2 ** 63, 0, 9131, 11016, -719528]
    c["L"] = nulls([pool[int(v)] for v in rng.integers(0, len(pool), n)], 0.1)
    c["g"] = nulls([int(v) for v in rng.integers(0, 5, n)], 0.1)
    c["p"] = nulls([int(v) for v in rng.integers(-10 ** 6, 10 ** 6, n)], 0.1)
    # the int32 ends, one step from leaving int32, at every size that has the rows
    for row, d, k in ((1, I32_MAX, 1), (3, I32_MIN, -1), (5, I32_MAX, 0), (7, I32_MIN, 0)):
        if row < n:
            c["d"][row], c["k"][row] = d, k
    return c


def arrow_table(c, names):
    arrays = []
    for name in names:
        if name == "p":
            arrays.append(pa.array([None if v is None else decimal.Decimal(v).scaleb(-2) for v in c[name]], ARROW[name]))
        elif ARROW[name] == pa.date32():
            arrays.append(pa.array(c[name], pa.int32()).cast(pa.date32()))
        else:
            arrays.append(pa.array(c[name], ARROW[name]))
    return pa.table(arrays, names=names)


def write_stripes(path, table, stripes):
    orc.write_table(table, path, compression="uncompressed", row_index_stride=1000, stripe_size=(64 << 20) if stripes == 1 else 1024)
    assert orc.ORCFile(path).nstripes == (1 if stripes == 1 else (table.num_rows + 1023) // 1024)
    return path


class File:
    def __init__(self, tmpdir, n, stripes=1, tag="f"):
        self.n, self.names = n, list(SCHEMA)
        self.c = make_columns(n)
        self.rows = [{k: self.c[k][i] for k in self.names} for i in range(n)]
        self.path = write_stripes(str(tmpdir / ("%s%d.orc" % (tag, n))), arrow_table(self.c, self.names), stripes)

    def builder(self, exprs=None, prefetch=0):
        b = ArrowReaderBuilder.try_new(self.path, ctx()).with_batch_size(BATCH).with_prefetch(prefetch)
        return b.with_computed_columns(exprs) if exprs else b

    def model(self, e):
        return M.computed_column(e, SCHEMA, self.rows)


def ints(table, name):
    t = table.column(name).type
    if pa.types.is_date(t):
        return table.column(name).cast(pa.int32()).to_pylist()
    return table.column(name).to_pylist()


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    return File(tmp_path_factory.mktemp("date_part"), 3 * 1024 + 1, stripes=4, tag="big")  # four stripes, the last of ONE row


@pytest.mark.parametrize("n, stripes", [(1, 1), (63, 1), (64, 1), (65, 1), (1024, 1), (1025, 1), (2049, 1), (3073, 4)])
def test_rows_against_the_model(tmp_path, n, stripes):
    f = File(tmp_path, n, stripes=stripes)
    names = list(EXPRS)  # eight computed columns at once, all six parts among them
    reader = f.builder([(k, EXPRS[k]) for k in names]).build()
    batches = list(reader)
    for b in batches:
        b.validate(full=True)
        assert b.schema.names == f.names + names
        for k in names:
            assert b.schema.field(k).type == pa.int64() and b.schema.field(k).nullable
    table = concat_batches(batches)
    assert table.num_rows == n and ints(table, "d") == f.c["d"]
    over = 0
    for k in names:
        want, o = f.model(EXPRS[k])
        over += o
        assert ints(table, k) == want, k
    assert reader.computed_overflow_rows() == over
    if n >= 64:
        assert over > 0  # the operands d + k and L do reach beyond int32
        got_y = dict(zip(ints(table, "d"), ints(table, "y")))
        assert got_y[I32_MAX] == 5881580 and got_y[I32_MIN] == -5877641


def test_no_present_stream_and_the_device_output_path(big):
    exprs = [("y", year("dn")), ("w", day_of_week("dn")), ("n", day_of_year(col("dn") - col("id")))]
    host = concat_batches(list(big.builder(exprs).with_projection(["id", "dn"]).build()))
    for k, e in exprs:
        want, over = big.model(e)
        assert ints(host, k) == want and None not in want and over == 0, k
    reader = big.builder([(k, EXPRS[k]) for k in EXPRS]).with_projection(["id", "d", "k", "L"]).with_device_output().build()
    dev = concat_batches([b.to_pyarrow() for b in reader])
    assert reader.d2h_bytes() == 0
    over = 0
    for k in EXPRS:
        want, o = big.model(EXPRS[k])
        over += o
        assert ints(dev, k) == want, k
    assert over > 0 and reader.computed_overflow_rows() == over


def test_poison_and_read_ahead(big, monkeypatch):
    monkeypatch.setenv("ORCGPU_POISON", "0xA5")  # a value or validity word left unwritten shows
    for prefetch in (0, 2):
        table = concat_batches(list(big.builder([(k, EXPRS[k]) for k in EXPRS], prefetch=prefetch).build()))
        for k in EXPRS:
            assert ints(table, k) == big.model(EXPRS[k])[0], (k, prefetch)


def kept_by(big, lhs, op, rhs, among):
    """the model's kept rows of `among`, and its overflow count there"""
    keep, over = [], 0
    for i in among:
        t, o = M.filter_leaf(lhs, op, rhs, big.rows[i], SCHEMA)
        over += 1 if o else 0
        if t is True:
            keep.append(i)
    return keep, over


def test_filter_leaves_under_a_selection_with_pruning_on_and_off(big):
    sel = [(100, False), (30, True), (900, False), (70, True), (1200, False), (500, True), (273, False)]  # (rows, skip), to the file's end
    assert sum(count for count, _ in sel) == big.n
    # the rows the selection hands out, stripe by stripe (tests/selection_model.py): the leaf is evaluated, and its overflows counted, on those
    stripe_rows = [1024, 1024, 1024, 1]
    picked = [1024 * s + i for s, ranges in enumerate(SM.file_batches(sel, stripe_rows, BATCH)) for start, length in ranges for i in range(start, start + length)]
    assert picked == [i for at, (count, skip) in zip(np.cumsum([0] + [c for c, _ in sel[:-1]]), sel) if not skip for i in range(at, at + count)]
    y0 = M.part_of(big.c["ds"][1], M.YEAR)
    # (lhs, op, rhs, whether the operand leaves int32 on some rows: rows 1 and 3 for d + k, a third of the Long's values)
    cases = [(year("ds"), "=", y0, False), (month("d"), "<", quarter("d") * 3, False), (year(col("d") + col("k")), ">=", 2000, True),
             (day_of_week("L"), "=", day_of_week("d"), True)]
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
                assert reader.filter_overflow_rows() == over, (pred, use_sel, prune)  # (under the selection: of the rows it hands out)
            assert (over > 0) == overflows, (pred, use_sel)  # the two that overflow do so with and without the selection
    # the .eq spelling, and NOT over a leaf: UNKNOWN stays out on both sides
    t = concat_batches(list(big.builder().with_row_filter(year("ds").eq(y0), prune=True).build()))
    assert t.column("id").to_pylist() == kept_by(big, year("ds"), "=", y0, range(big.n))[0]
    t = concat_batches(list(big.builder().with_row_filter(P.not_(year(col("d") + col("k")).eq(2000)), prune=False).build()))
    assert t.column("id").to_pylist() == kept_by(big, year(col("d") + col("k")), "!=", 2000, range(big.n))[0]
    assert kept_by(big, year(col("d") + col("k")), ">=", 2000, range(big.n))[1] > 0


def model_aggs(big, idx, y0):
    """SUM(year(ds)), AVG(day_of_year(ds)), COUNT(*) WHERE year(ds) = y0, SUM(year(ds) * p) over the rows idx"""
    ys = [v for v in (M.agg_row(year("ds"), SCHEMA, big.rows[i]) for i in idx) if v is not None]
    ns = [v for v in (M.agg_row(day_of_year("ds"), SCHEMA, big.rows[i]) for i in idx) if v is not None]
    yp = [v for v in (M.agg_row(year("ds") * col("p"), SCHEMA, big.rows[i]) for i in idx) if v is not None]
    return [sum(ys) if ys else None, AEM.avg_int(sum(ns), len(ns)) if ns else None, sum(1 for v in ys if v == y0),
            decimal.Decimal(sum(yp)).scaleb(-2) if yp else None]


def specs_for(y0):
    return [Agg.sum(year("ds")), Agg.avg(day_of_year("ds")), Agg.count_rows().where(year("ds").eq(y0)), Agg.sum(year("ds") * col("p"))]


def test_aggregates_plain_and_grouped(big):
    y0 = M.part_of(big.c["ds"][1], M.YEAR)
    got = big.builder().aggregate(specs_for(y0))
    assert got == model_aggs(big, range(big.n), y0) and got[2] > 0
    groups = {}
    for i, r in enumerate(big.rows):
        groups.setdefault(r["g"], []).append(i)
    for limit in (None, 1024):
        res = big.builder().aggregate(specs_for(y0), group_by=["g"], max_groups=limit)
        assert [k[0] for k, _ in res] == list(groups)
        for (k, vals), idx in zip(res, groups.values()):
            assert vals == model_aggs(big, idx, y0), (limit, k)
    # a Date column over the full range, in aggregate mode: loaded by its decoded width, int32 ends included
    want = [v for v in (M.agg_row(year("d"), SCHEMA, r) for r in big.rows) if v is not None]
    assert big.builder().aggregate([Agg.sum(year("d")), Agg.sum(year(col("d") + 0))]) == [sum(want), sum(want)]
    # an operand outside int32 is AGG_OVERFLOW, as an operation that leaves 128 bits is
    assert any(M.agg_row(year("L"), SCHEMA, r) == AEM.ROW_OVERFLOW for r in big.rows)
    with pytest.raises(OverflowError):
        big.builder().aggregate([Agg.sum(year("L"))])
    with pytest.raises(OverflowError):
        big.builder().aggregate([Agg.avg(month(col("d") + col("k")))])
    # outside a date part a Date stays what the aggregates refuse
    with pytest.raises(capi.OrcGpuError) as e:
        big.builder().aggregate([Agg.sum(col("d") + 1)])
    assert e.value.code == 6 and "does not take column 'd'" in str(e.value)


@pytest.mark.parametrize("keys", [["yr"], ["yr", "mo"]])
@pytest.mark.parametrize("limit", [None, 1024])
def test_group_by_computed_year_and_month_on_both_paths(big, keys, limit):
    exprs = {"yr": year("ds"), "mo": month("ds")}
    vals = {k: big.model(exprs[k])[0] for k in keys}
    groups = {}
    for i in range(big.n):
        groups.setdefault(tuple(vals[k][i] for k in keys), []).append(i)
    assert (len(groups) > 60) == (len(keys) == 2) and len(groups) <= 256
    res = big.builder({k: exprs[k] for k in keys}).aggregate([Agg.count_rows(), Agg.sum("p"), Agg.sum(day("ds"))], group_by=keys, max_groups=limit)
    assert [k for k, _ in res] == list(groups)
    for (k, got), idx in zip(res, groups.values()):
        ps = [big.rows[i]["p"] for i in idx if big.rows[i]["p"] is not None]
        ds = [v for v in (M.agg_row(day("ds"), SCHEMA, big.rows[i]) for i in idx) if v is not None]
        assert got == [len(idx), decimal.Decimal(sum(ps)).scaleb(-2) if ps else None, sum(ds) if ds else None], (keys, limit, k)


def test_top_k_by_a_computed_year_then_a_second_key(big):
    want_y, _ = big.model(year("d"))
    for desc, nf in ((False, False), (True, True), (True, False)):
        got = big.builder({"yr": year("d")}).top_k([SortKey("yr", descending=desc, nulls_first=nf), SortKey("id", descending=True)], 40)

        def order(i):
            v = want_y[i]
            null_rank = (0 if nf else 1) if v is None else (1 if nf else 0)
            return (null_rank, 0 if v is None else (-v if desc else v), -i)
        exp = sorted(range(big.n), key=order)[:40]
        assert got.column("id").to_pylist() == exp and ints(got, "yr") == [want_y[i] for i in exp], (desc, nf)


def test_collect_keys_of_a_computed_year_used_in_in_set(big):
    want, _ = big.model(year("ds"))
    small = [i for i in range(1, big.n) if i % 97 == 0][:4]  # four build rows: at most four of the seven years, a proper subset
    ks = big.builder({"yr": year("ds")}).with_row_filter(P.in_list("id", [V.Int64(i) for i in small]), prune=False).collect_keys("yr", max_keys=1 << 10)
    try:
        keys = {want[i] for i in small if want[i] is not None}
        assert len(ks) == len(keys) and 1 <= len(keys) <= 4
        t = concat_batches(list(big.builder({"yr": year("ds")}).with_row_filter(P.in_set("yr", ks), prune=False).build()))
        assert t.column("id").to_pylist() == [i for i in range(big.n) if want[i] in keys]
    finally:
        ks.close()


def test_collect_map_with_a_computed_year_looked_up_from_a_probe_file(big, tmp_path):
    """orders -> a key map of year(o_orderdate); the probe side groups by the looked-up year: the Q9 shape"""
    want_y, _ = big.model(year("ds"))
    want_ym, _ = big.model(year("ds") * 100 + month("ds"))
    km = big.builder({"o_year": year("ds"), "o_ym": year("ds") * 100 + month("ds")}).collect_map("id", ["o_year", "o_ym"], max_keys=1 << 12)
    try:
        assert len(km) == big.n
        rng = np.random.default_rng(3)
        fk = [None if k % 50 == 7 else int(v) for k, v in enumerate(rng.integers(-5, big.n + 5, 1500))]  # some keys miss, some are NULL
        path = str(tmp_path / "probe.orc")
        orc.write_table(pa.table({"rid": pa.array(range(1500), pa.int64()), "fk": pa.array(fk, pa.int64())}), path, compression="uncompressed")
        b = ArrowReaderBuilder.try_new(path, ctx()).with_batch_size(BATCH).with_prefetch(0).with_lookup_columns(km, "fk", {"yr": "o_year", "ym": "o_ym"})
        t = concat_batches(list(b.build()))
        look = lambda vals: [vals[k] if k is not None and 0 <= k < big.n else None for k in fk]
        assert ints(t, "yr") == look(want_y) and ints(t, "ym") == look(want_ym)
        b = ArrowReaderBuilder.try_new(path, ctx()).with_batch_size(BATCH).with_prefetch(0).with_lookup_columns(km, "fk", {"yr": "o_year"})
        res = b.aggregate([Agg.count_rows()], group_by=["yr"])
        groups = {}
        for v in look(want_y):
            groups[v] = groups.get(v, 0) + 1
        assert [(k[0], v[0]) for k, v in res] == list(groups.items())
    finally:
        km.close()


def test_c_side_refusals(big):
    def refused(run, code, *fragments):
        with pytest.raises(capi.OrcGpuError) as e:
            run()
        assert e.value.code == code and all(f in str(e.value) for f in fragments), str(e.value)
    refused(lambda: list(big.builder({"r": year("p")}).build()), 6, "year()", "column 'p'", "computed column 'r'")
    refused(lambda: list(big.builder({"r": month(col("d") + 1.5)}).build()), 6, "month()", "FLOAT64 literal")
    refused(lambda: big.builder().aggregate([Agg.sum(day_of_year("p"))]), 6, "day_of_year()", "column 'p'")
    refused(lambda: list(big.builder().with_row_filter(year("p").eq(1995), prune=False).build()), 6, "row filter:", "year()", "column 'p'")
    bad = year("d")
    bad.part = 6  # (what Python's builders never make)
    refused(lambda: list(big.builder({"r": bad}).build()), 101, "names no part")
    refused(lambda: list(big.builder().with_row_filter(bad.eq(1), prune=False).build()), 101, "names no part")
    refused(lambda: big.builder().aggregate([Agg.sum(bad)]), 101, "names no part")
