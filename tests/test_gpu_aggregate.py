"""COUNT, SUM, MIN, MAX and SUM_PRODUCT over the kept rows on the GPU (orcgpu_result_aggregate, orcgpu_reader_set_aggregates /
orcgpu_reader_aggregate: device/agg_kernels.hip) against the model of tests/agg_model.py.  Files are written with pyarrow.orc and
with this project's writer; the expected values come from the table that was written, never from a read of it."""
import ctypes as C
import decimal
import io
import math
import struct

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import agg_model as AM
import selection_model as SM
from orc_rust_amd import aggregate as A
from orc_rust_amd import capi, gen
from orc_rust_amd.aggregate import Agg
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.arrow_writer import ArrowWriterBuilder
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

pytestmark = pytest.mark.gpu

D = decimal.Decimal
BATCH = 1024
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 70_001)   # across a word of the keep mask, a batch and several blocks
NULLS = (0.0, 0.3, 1.0)
T0 = 1_600_000_000 * 10 ** 9
INT_COLS, FLOAT_COLS, DEC_COLS, TS_COLS = ("i8", "i16", "i32", "i64"), ("f32", "f64"), ("dec", "dec38"), ("ts", "tsi")
VALUE_COLS = INT_COLS + FLOAT_COLS + DEC_COLS + TS_COLS + ("date", "b")
ALL_COLS = ("id", "g") + VALUE_COLS + ("s",)
MISMATCHED, UNSUPPORTED, INVALID = 6, 7, 101
_CTX = None
_TABLES, _FILES = {}, {}


def ctx():
    global _CTX
    if _CTX is None:
        _CTX = capi.Context()
    return _CTX


def make_table(n, null_frac, seed=11):
    key = (n, null_frac)
    if key in _TABLES:
        return _TABLES[key]
    rng = np.random.default_rng(seed + n)

    def nulls(values):
        mask = rng.random(n) < null_frac if null_frac < 1.0 else np.ones(n, bool)
        return [None if m else v for v, m in zip(values, mask)]

    cols = {
        "id": pa.array(np.arange(n, dtype=np.int64)),
        "g": pa.array(rng.integers(-3, 4, n), pa.int64()),
        "i8": pa.array(nulls(rng.integers(-128, 128, n).tolist()), pa.int8()),
        "i16": pa.array(nulls(rng.integers(-2 ** 15, 2 ** 15, n).tolist()), pa.int16()),
        "i32": pa.array(nulls(rng.integers(-2 ** 31, 2 ** 31, n).tolist()), pa.int32()),
        "i64": pa.array(nulls(rng.integers(-2 ** 63, 2 ** 63 - 1, n).tolist()), pa.int64()),
        "f32": pa.array(nulls((rng.standard_normal(n) * 100).astype(np.float32).tolist()), pa.float32()),
        "f64": pa.array(nulls((rng.standard_normal(n) * 1e9).tolist()), pa.float64()),
        "dec": pa.array(nulls([D(int(x)).scaleb(-2) for x in rng.integers(-10 ** 14, 10 ** 14, n)]), pa.decimal128(15, 2)),
        "dec38": pa.array(nulls([D(int(a) * 2 ** 64 + int(b)) for a, b in zip(rng.integers(-2 ** 40, 2 ** 40, n), rng.integers(0, 2 ** 62, n))]), pa.decimal128(38, 0)),
        "ts": pa.array(nulls((T0 + 1000 * rng.integers(0, 10 ** 12, n)).tolist()), pa.timestamp("ns")),
        "tsi": pa.array(nulls((T0 + 1000 * rng.integers(0, 10 ** 12, n)).tolist()), pa.timestamp("ns", tz="UTC")),
        "date": pa.array(nulls(rng.integers(-20000, 20000, n).tolist()), pa.date32()),
        "b": pa.array(nulls((rng.random(n) < 0.5).tolist()), pa.bool_()),
        "s": pa.array(nulls(["row %d" % x for x in range(n)]), pa.string()),
    }
    _TABLES[key] = pa.table(cols)
    return _TABLES[key]


def specs_for(names):
    out = [Agg.count_rows()]
    for c in names:
        out.append(Agg.count(c))
        if c in INT_COLS + FLOAT_COLS + DEC_COLS:
            out.append(Agg.sum(c))
        if c in VALUE_COLS:
            out += [Agg.min(c), Agg.max(c)]
    for a, b in (("i8", "i64"), ("i32", "i32"), ("f32", "f64"), ("dec", "dec")):
        if a in names and b in names:
            out.append(Agg.sum_product(a, b))
    assert len(out) <= 64
    return out


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    capi.load()  # (sets TZDIR where the system has no tz database: pyarrow's ORC writer needs one for the Timestamp columns)
    return tmp_path_factory.mktemp("aggregate")


def pyarrow_file(tmpdir, n, null_frac):
    key = ("pa", n, null_frac)
    if key not in _FILES:
        path = str(tmpdir / ("pa%d_%d.orc" % (n, int(null_frac * 100))))
        orc.write_table(make_table(n, null_frac), path, compression="uncompressed", row_index_stride=1000, stripe_size=64 << 20)
        assert n == 0 or orc.ORCFile(path).nstripes == 1
        _FILES[key] = path
    return _FILES[key]


def own_file(table, stripes=1, stride=0):
    """`table` through this project's writer (no Date column: it writes none), cut into `stripes` stripes of about equal rows"""
    out = io.BytesIO()
    w = ArrowWriterBuilder(out, table.schema, ctx=ctx()).with_row_index_stride(stride).try_build()
    n = table.num_rows
    cuts = [n * k // stripes for k in range(stripes + 1)]
    rows = []
    for a, b in zip(cuts, cuts[1:]):
        for batch in table.slice(a, b - a).to_batches():
            w.write(batch)
        w.flush_stripe()
        rows.append(b - a)
    w.close()
    w.free()
    return out.getvalue(), rows


def builder(src, names, pred=None, selection=None, prefetch=0, prune=False, precision=None):
    b = ArrowReaderBuilder.try_new(src, ctx()).with_batch_size(BATCH).with_prefetch(prefetch).with_projection(list(names))
    if precision is not None:
        b = b.with_timestamp_precision(precision)
    if selection is not None:
        b = b.with_row_selection(selection)
    if pred is not None:
        b = b.with_row_filter(pred, prune=prune)
    return b


def drain(reader, specs):
    """(values, (rows seen, rows kept), bytes copied back) of an aggregating reader; a set overflow flag becomes AM.OVERFLOW"""
    try:
        raw = reader.aggregate(raw=True)
        return [AM.OVERFLOW if v.overflow else A.value_of(v, s) for v, s in zip(raw, specs)], reader.filter_rows(), reader.d2h_bytes()
    finally:
        reader.close()


def run(src, names, specs, **kw):
    return drain(builder(src, names, **kw).aggregating_reader(specs), specs)


def check(table, specs, got, keep, what, ts_unit="ns"):
    want = AM.aggregate(table, specs, keep=keep, ts_unit=ts_unit)
    for s, g, w in zip(specs, got, want):
        if s.op in (A.SUM, A.SUM_PRODUCT) and isinstance(w, float) and w == w and not math.isinf(w):
            bound = AM.float_bound(AM.float_terms(table, s, keep))
            print(what, s, "got %r fsum %r bound %r" % (g, w, bound))
            assert isinstance(g, float) and abs(g - w) <= bound, (what, s, g, w, bound)
        else:
            assert AM.same(g, w), (what, s, g, w)


def selection_over(n):
    """skip 37, select 200, ... over n rows: runs shorter than a batch, ends inside words and across batches"""
    out, left, skip = [], n, True
    while left > 0:
        k = min(left, 37 if skip else 200)
        out.append((k, skip))
        left -= k
        skip = not skip
    return out


def arms(n):
    """the five kept-row arms: (name, predicate, selection)"""
    return [("none", None, None), ("nothing", P.lt("id", V.Int64(-1)), None), ("everything", P.gte("id", V.Int64(0)), None),
            ("half", P.lt("g", V.Int64(0)), None), ("in+selection", P.in_list("g", [V.Int64(-2), V.Int64(0), V.Int64(3)]), selection_over(n))]


@pytest.mark.parametrize("null_frac", NULLS)
@pytest.mark.parametrize("n", SIZES)
def test_every_kind_size_and_arm_pyarrow_file(tmpdir, n, null_frac):
    table = make_table(n, null_frac)
    path = pyarrow_file(tmpdir, n, null_frac)
    specs = specs_for(ALL_COLS)
    for name, pred, sel in arms(n):
        if n == 0 and sel is not None:
            sel = [(5, True), (5, False)]
        got, (seen, kept), d2h = run(path, ALL_COLS, specs, pred=pred, selection=sel)
        keep = AM.kept_mask(table, pred, sel, BATCH)
        check(table, specs, got, keep, (n, null_frac, name))
        assert d2h == 0
        assert (seen, kept) == (int(AM.kept_mask(table, None, sel, BATCH).sum()), int(keep.sum())), (name, seen, kept)


@pytest.mark.parametrize("null_frac", NULLS)
@pytest.mark.parametrize("n", (1, 65, 1025, 2049))
def test_every_kind_own_writer(n, null_frac):
    table = make_table(n, null_frac).drop_columns(["date"])
    names = [c for c in ALL_COLS if c != "date"]
    data, _ = own_file(table)
    specs = specs_for(names)
    for name, pred, sel in arms(n):
        got, _, d2h = run(data, names, specs, pred=pred, selection=sel)
        check(table, specs, got, AM.kept_mask(table, pred, sel, BATCH), (n, null_frac, name))
        assert d2h == 0


def test_integer_sum_at_the_extremes_is_exact():
    n = 70_001
    big, small = 2 ** 63 - 1, -2 ** 63
    rng = np.random.default_rng(2)
    mixed = np.where(rng.random(n) < 0.5, big, small).astype(np.int64)
    table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "max": pa.array(np.full(n, big, dtype=np.int64)), "min": pa.array(np.full(n, small, dtype=np.int64)),
                      "mixed": pa.array(mixed)})
    data, _ = own_file(table)
    specs = [Agg.sum("max"), Agg.sum("min"), Agg.sum("mixed"), Agg.sum_product("max", "max"), Agg.sum_product("min", "max"), Agg.min("mixed"), Agg.max("mixed")]
    got, _, _ = run(data, table.column_names, specs)
    assert got[0] == n * big and got[1] == n * small and got[2] == sum(int(x) for x in mixed)
    assert got[3] == AM.OVERFLOW and got[4] == AM.OVERFLOW       # 70 001 * 2^126 leaves int128 (the 192-bit accumulator holds it)
    assert got[5:] == [small, big]
    # INT64_MIN * INT64_MIN: one row is 2^126, two rows are 2^127 -- the first value outside int128
    one, _, _ = run(data, table.column_names, [Agg.sum_product("min", "min")], pred=P.lt("id", V.Int64(1)))
    two, _, _ = run(data, table.column_names, [Agg.sum_product("min", "min"), Agg.sum_product("min", "max")], pred=P.lt("id", V.Int64(2)))
    assert one == [2 ** 126] and two == [AM.OVERFLOW, 2 * small * big]
    with pytest.raises(OverflowError) as e:
        builder(data, table.column_names).aggregate([Agg.sum_product("min", "min")])
    assert "sum_product('min', 'min')" in str(e.value)


def test_decimal_sum_at_the_edge_of_38_digits():
    n = 1025
    vals = [D(10 ** 38 - 1 - (n - 2))] + [D(1)] * (n - 1)            # all but the last row: 10^38 - 1; with it: 10^38
    neg = [v.copy_negate() for v in vals]     # (unary minus would round to the context's 28 digits)
    table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "d": pa.array(vals, pa.decimal128(38, 0)), "m": pa.array(neg, pa.decimal128(38, 0))})
    data, _ = own_file(table)
    got, _, _ = run(data, table.column_names, [Agg.sum("d"), Agg.sum("m"), Agg.max("d"), Agg.min("m")], pred=P.lt("id", V.Int64(n - 1)))
    assert got == [D(10 ** 38 - 1), D(-(10 ** 38 - 1)), vals[0], neg[0]]
    got, _, _ = run(data, table.column_names, [Agg.sum("d"), Agg.sum("m"), Agg.count("d")])
    assert got == [AM.OVERFLOW, AM.OVERFLOW, n]
    # an operand of a product beyond a signed 64-bit word: the sticky flag
    got, _, _ = run(data, table.column_names, [Agg.sum_product("d", "d")], pred=P.gt("id", V.Int64(0)))
    assert got == [D(n - 1)]
    got, _, _ = run(data, table.column_names, [Agg.sum_product("d", "d")])
    assert got == [AM.OVERFLOW]


def test_q6_expression_decimal_15_2():
    n = 2049
    rng = np.random.default_rng(4)
    price = pa.array([D(int(x)).scaleb(-2) for x in rng.integers(90_000, 10_500_000, n)], pa.decimal128(15, 2))
    disc = pa.array([None if k % 11 == 0 else D(int(x)).scaleb(-2) for k, x in enumerate(rng.integers(0, 11, n))], pa.decimal128(15, 2))
    t = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "l_extendedprice": price, "l_discount": disc})
    data, _ = own_file(t)
    pred = P.and_([P.gte("l_discount", V.Decimal128(D("0.05"))), P.lte("l_discount", V.Decimal128(D("0.07")))])
    spec = [Agg.sum_product("l_extendedprice", "l_discount"), Agg.count_rows()]
    got, _, _ = run(data, t.column_names, spec, pred=pred)
    want = AM.aggregate(t, spec, pred)
    assert got == want and isinstance(got[0], D) and got[0].as_tuple().exponent == -4 and got[1] > 0


def f64_file(values, extra=None):
    cols = {"id": pa.array(np.arange(len(values), dtype=np.int64)), "x": pa.array(values, pa.float64())}
    cols.update(extra or {})
    t = pa.table(cols)
    return t, own_file(t)[0]


def test_float_sums_nan_inf_and_determinism():
    nan, inf = math.nan, math.inf
    n = 70_001
    rng = np.random.default_rng(8)
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)).tolist()      # sixteen orders of magnitude: the order of summation shows
    t, data = f64_file(x, {"y": pa.array(rng.standard_normal(n).astype(np.float32).tolist(), pa.float32())})
    specs = [Agg.sum("x"), Agg.sum("y"), Agg.sum_product("x", "y")]
    runs = [builder(data, t.column_names).aggregate(specs, raw=True) for _ in range(2)]
    check(t, specs, [v.f for v in runs[0]], np.ones(n, bool), "finite")
    assert [struct.pack("<d", v.f) for v in runs[0]] == [struct.pack("<d", v.f) for v in runs[1]]   # the same 8 bytes
    for values, want_nan in (([1.0, nan, 2.0] + [0.5] * 200, True), ([inf, 1.0, -inf] + [0.5] * 200, True), ([inf, 1.0, 2.0], False)):
        t, data = f64_file(values)
        got, _, _ = run(data, t.column_names, [Agg.sum("x"), Agg.sum_product("x", "x")])
        assert (got[0] != got[0]) == want_nan and (want_nan or got[0] == inf)
        assert AM.same(got[0], AM.aggregate(t, [Agg.sum("x")])[0])


def test_min_max_with_nan_and_zeros():
    nan = math.nan
    some = [3.0, nan, -7.5, None, nan, 2.0] * 40
    t, data = f64_file(some, {"allnan": pa.array([nan, None] * 120, pa.float64()), "z": pa.array([-0.0, 0.0, None] * 80, pa.float64()),
                              "nul": pa.array([None] * 240, pa.float64())})
    specs = [Agg.min("x"), Agg.max("x"), Agg.min("allnan"), Agg.max("allnan"), Agg.min("z"), Agg.max("z"), Agg.min("nul"), Agg.max("nul"), Agg.count("allnan")]
    got, _, _ = run(data, t.column_names, specs)
    assert got[:2] == [-7.5, 3.0]
    assert got[2] != got[2] and got[3] != got[3]        # every kept non-null value is NaN: NaN, not NULL
    assert got[4] == 0.0 and got[5] == 0.0              # (-0.0 and 0.0 compare equal: either may come back)
    assert got[6:] == [None, None, 120]
    check(t, specs, got, np.ones(240, bool), "nan")
    got, _, _ = run(data, t.column_names, specs[:4], pred=P.lt("id", V.Int64(2)))     # rows 0, 1: 3.0 and NaN | NaN and null
    assert got[:2] == [3.0, 3.0] and got[2] != got[2]


def test_timestamps_in_ns_and_us(tmpdir):
    n = 1025
    table = make_table(n, 0.3)
    path = pyarrow_file(tmpdir, n, 0.3)
    specs = [Agg.min("ts"), Agg.max("ts"), Agg.min("tsi"), Agg.max("tsi"), Agg.count("ts")]
    for unit in ("ns", "us"):
        got, _, _ = run(path, ["id", "ts", "tsi"], specs, precision=unit)
        check(table, specs, got, np.ones(n, bool), unit, ts_unit=unit)
        assert [g.units for g in got[:4]] == [unit] * 4


def three_stripes(n=3 * 1025 + 7, null_frac=0.3, stride=0):
    table = make_table(n, null_frac).drop_columns(["date"])
    data, rows = own_file(table, stripes=3, stride=stride)
    assert orc.ORCFile(io.BytesIO(data)).nstripes == 3
    return table, data, rows


def test_reader_merges_stripes_in_order():
    table, data, rows = three_stripes()
    names = [c for c in ALL_COLS if c != "date"]
    specs = specs_for(names)
    pred = P.lt("g", V.Int64(1))
    whole = AM.kept_mask(table, pred)
    for prefetch in (0, 2):
        got, (seen, kept), d2h = run(data, names, specs, pred=pred, prefetch=prefetch)
        check(table, specs, got, whole, ("stripes", prefetch))
        assert (seen, kept, d2h) == (table.num_rows, int(whole.sum()), 0)
    # ... which is the merge of the stripes' own results: exact ones add up, MIN / MAX fold
    parts, at = [], 0
    for k in rows:
        parts.append(AM.aggregate(table.slice(at, k), specs, pred))
        at += k
    for s, g, per in zip(specs, got, zip(*parts)):
        real = [p for p in per if p is not None]
        if isinstance(g, float):
            continue
        if real and isinstance(real[0], D):     # (exactly: as unscaled integers at the common scale)
            e = real[0].as_tuple().exponent
            real = [int(p.scaleb(-e, AM.EXACT)) for p in real]
            g = int(g.scaleb(-e, AM.EXACT))
        if s.op in (A.COUNT_ROWS, A.COUNT, A.SUM, A.SUM_PRODUCT):
            assert g == (sum(real) if real else None), s
        else:
            assert g == ((max if s.op == A.MAX else min)(real) if real else None), s
    # a shard reads its stripes only: rank 0 of 2 has stripes 0 and 2
    got, (seen, _), _ = drain(builder(data, names).with_shard(0, 2).aggregating_reader(specs), specs)
    keep = np.zeros(table.num_rows, bool)
    keep[:rows[0]] = True
    keep[rows[0] + rows[1]:] = True
    check(table, specs, got, keep, "shard")
    assert seen == rows[0] + rows[2]


def test_reader_pruning_on_and_off_gives_the_same():
    table, data, rows = three_stripes(stride=1000)
    names = ["id", "g", "i64", "f64", "dec"]
    specs = specs_for(names)
    pred = P.and_([P.gte("id", V.Int64(1500)), P.lt("id", V.Int64(2600))])
    keep = AM.kept_mask(table, pred)
    seen = {}
    for prune in (False, True):
        got, (seen[prune], kept), d2h = run(data, names, specs, pred=pred, prune=prune, prefetch=2)
        check(table, specs, got, keep, ("prune", prune))
        assert d2h == 0 and kept == int(keep.sum())
    assert seen[True] < seen[False] == table.num_rows      # pruning read fewer rows for the same answer


def test_next_batch_is_refused_and_aggregate_still_works():
    table, data, _ = three_stripes()
    specs = [Agg.count_rows(), Agg.sum("i64")]
    r = builder(data, ["id", "i64"]).aggregating_reader(specs)
    with pytest.raises(capi.OrcGpuError) as e:
        next(r)
    assert e.value.code == INVALID and "aggregate" in str(e.value)
    assert r.aggregate() == AM.aggregate(table, specs)
    with pytest.raises(StopIteration):      # drained: ORCGPU_END_OF_FILE
        r.aggregate()
    r.close()
    plain = builder(data, ["id", "i64"]).build()
    plain._agg_specs = specs
    with pytest.raises(capi.OrcGpuError) as e:
        plain.aggregate()
    assert e.value.code == INVALID
    assert sum(b.num_rows for b in plain) == table.num_rows     # ... and that reader reads on as it always did
    plain.close()


def stripe_result(n, batch=1000, seed=3):
    rng = np.random.default_rng(seed)
    present = (rng.random(n) > 0.3).astype(np.uint8)
    vals = rng.integers(-50, 50, int(present.sum())).astype(np.int64)
    ids = np.arange(n, dtype=np.int64)
    cols = [{"column_id": 1, "orc_type": 4, "encoding": 2}, {"column_id": 2, "orc_type": 4, "encoding": 2}]
    streams = [(1, 1, gen.rle2(ids, signed=True)), (2, 0, gen.boolean(present)), (2, 1, gen.rle2(vals, signed=True))]
    full = np.zeros(n, dtype=np.int64)
    full[present == 1] = vals
    c = ctx()
    staged = c.stage(n, streams, cols, batch_size=batch)
    res = c.decode([staged])[0]
    staged.free()
    table = pa.table({"id": pa.array(ids), "v": pa.array([int(x) if p else None for x, p in zip(full, present)], pa.int64())})
    return res, table


def batches_of(res):
    out = []
    for b in range(res.n_batches):
        for col in range(2):
            v = res.batch(b, col)
            out.append((v["length"], v["values"], v["validity"], v["null_count"]))
    return out


def test_result_aggregate_leaves_the_result_and_the_filter_alone():
    n, batch = 4097, 1000
    c = ctx()
    specs = [Agg.count_rows(), Agg.count("v"), Agg.sum("v"), Agg.min("v"), Agg.max("v"), Agg.sum_product("v", "id")]
    pred = P.and_([P.gt("v", V.Int64(10)), P.gte("id", V.Int64(64))])
    res, table = stripe_result(n, batch)
    before = batches_of(res)
    assert c.result_aggregate(res, specs, ["id", "v"]) == AM.aggregate(table, specs)
    assert c.result_aggregate(res, specs, ["id", "v"], pred) == AM.aggregate(table, specs, pred)
    assert c.result_aggregate(res, specs, ["id", "v"], pred) == AM.aggregate(table, specs, pred)      # any number of times
    assert batches_of(res) == before                                                               # byte for byte as it was
    # a selected result: the selection's rows
    sel = [(100, True), (900, False), (1000, True), (700, False)]
    res.select(sel)
    keep = np.zeros(n, bool)
    for s, k in SM.stripe_batches(SM.normalise(sel), n, batch):
        keep[s:s + k] = True
    assert c.result_aggregate(res, specs, ["id", "v"]) == AM.aggregate(table, specs, keep=keep)
    keep_f = keep & AM.kept_mask(table, pred)
    assert c.result_aggregate(res, specs, ["id", "v"], pred) == AM.aggregate(table, specs, keep=keep_f)
    # the filter after it gives what it gives without it ...
    kept = c.result_filter(res, pred, ["id", "v"])
    res2, _ = stripe_result(n, batch)
    res2.select(sel)
    assert c.result_filter(res2, pred, ["id", "v"]) == kept == int(keep_f.sum())
    assert batches_of(res) == batches_of(res2)
    # ... and a filtered result is aggregated as the rows it now holds
    assert c.result_aggregate(res, specs, ["id", "v"]) == AM.aggregate(table, specs, keep=keep_f)
    assert batches_of(res) == batches_of(res2)
    res.free()
    res2.free()
    # nulls among the kept rows of a filtered result
    res, table = stripe_result(n, batch)
    nulls = P.or_([P.is_null("v"), P.lt("v", V.Int64(-40))])
    c.result_filter(res, nulls, ["id", "v"])
    assert c.result_aggregate(res, specs, ["id", "v"]) == AM.aggregate(table, specs, nulls)
    res.free()


def refused(b, specs, code, word):
    r = b.aggregating_reader(specs)
    with pytest.raises(capi.OrcGpuError) as e:
        r.aggregate()
    assert e.value.code == code and word in str(e.value), (specs, code, word, str(e.value))
    r.close()


def test_refusals_are_loud_and_name_the_column(tmpdir):
    n = 1025
    path = pyarrow_file(tmpdir, n, 0.3)
    for col in ("s", "date", "b", "ts", "tsi"):
        refused(builder(path, ALL_COLS), [Agg.sum(col)], MISMATCHED, "'%s'" % col)
    for op in (Agg.min, Agg.max):
        refused(builder(path, ALL_COLS), [op("s")], MISMATCHED, "'s'")
    refused(builder(path, ALL_COLS), [Agg.sum_product("i64", "f64")], MISMATCHED, "'f64'")
    refused(builder(path, ALL_COLS), [Agg.sum_product("dec", "i64")], MISMATCHED, "'i64'")
    refused(builder(path, ALL_COLS), [Agg.sum_product("i64", "date")], MISMATCHED, "'date'")
    for spec in (Agg.min("s"), Agg.max("s"), Agg.sum("s"), Agg.sum_product("s", "s")):
        refused(builder(path, ALL_COLS).with_dictionary_columns(["s"]), [spec], UNSUPPORTED, "'s'")
    for spec in (Agg.min("ts"), Agg.max("tsi")):      # Timestamp decoded to Decimal128(38, 9)
        sch = pa.schema([("id", pa.int64()), ("ts", pa.decimal128(38, 9)), ("tsi", pa.decimal128(38, 9))])
        refused(builder(path, ["id", "ts", "tsi"]).with_schema(sch), [spec], UNSUPPORTED, "'%s'" % spec.column)
    refused(builder(path, ALL_COLS), [Agg.sum("nope")], INVALID, "'nope'")
    refused(builder(path, ["id", "g"]), [Agg.sum("i64")], INVALID, "'i64'")        # not projected
    refused(builder(path, ALL_COLS), [Agg.sum_product("i64", "nope")], INVALID, "'nope'")
    bad = Agg.sum("i64")
    bad.op = 9
    refused(builder(path, ALL_COLS), [bad], INVALID, "unknown op")
    # COUNT takes everything, a dictionary column included
    got, _, _ = run(path, ALL_COLS, [Agg.count("s")])
    r = builder(path, ALL_COLS).with_dictionary_columns(["s"]).aggregating_reader([Agg.count("s"), Agg.count_rows()])
    assert r.aggregate() == [got[0], n]
    r.close()
    # the scale rule and a nested column
    st = pa.table({"id": pa.array([1, 2], pa.int64()), "st": pa.array([{"a": 1}, {"a": 2}], pa.struct([("a", pa.int64())])),
                   "d20": pa.array([D(1).scaleb(-20), D(2).scaleb(-20)], pa.decimal128(38, 20)),
                   "d18": pa.array([D(1).scaleb(-18), D(2).scaleb(-18)], pa.decimal128(38, 18))})
    data, _ = own_file(st)
    refused(builder(data, ["id", "st"]), [Agg.count_rows()], UNSUPPORTED, "'st'")
    refused(builder(data, ["d20"]), [Agg.sum_product("d20", "d20")], UNSUPPORTED, "'d20'")
    r = builder(data, ["d20", "d18"]).aggregating_reader([Agg.sum_product("d20", "d18")])      # 20 + 18 = 38: accepted
    assert r.aggregate() == [D(5).scaleb(-38)]
    r.close()
    # the C ABI itself: more than 64 specs and none (Python refuses both first), a column the result does not have
    res, _ = stripe_result(100)
    arr, out = (A.AggSpec * 65)(), (A.AggValue * 65)()
    names = (C.c_char_p * 2)(b"id", b"v")
    c = ctx()
    assert c.L.orcgpu_result_aggregate(c.h, res.h, None, 0, names, 2, arr, 65, out) == INVALID
    assert c.L.orcgpu_result_aggregate(c.h, res.h, None, 0, names, 2, arr, 0, out) == INVALID
    with pytest.raises(capi.OrcGpuError) as e:
        c.result_aggregate(res, [Agg.sum("w")], ["id", "v"])
    assert e.value.code == INVALID and "'w'" in str(e.value)
    res.free()
