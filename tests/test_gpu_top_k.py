"""ORDER BY ... LIMIT k on the GPU (orcgpu_result_top_k, orcgpu_reader_set_top_k / orcgpu_reader_top_k_order:
device/top_k_kernels.hip) against the model of tests/top_k_model.py, row for row and every column.  Files come from ArrowWriter and
pyarrow.orc as in test_gpu_aggregate.py, whose table builders are used as they are; the expected rows come from the table that was
written and the model's stable sort, never from a read."""
import ctypes as C
import decimal

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import agg_model as AM
import test_gpu_aggregate as TA
import top_k_model as M
from orc_rust_amd import capi
from orc_rust_amd.arrow_reader import concat_batches
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
from orc_rust_amd.top_k import SortKey, SortKeyStruct

pytestmark = pytest.mark.gpu

D = decimal.Decimal
BATCH = TA.BATCH
SIZES = TA.SIZES
UNSUPPORTED, INVALID, END_OF_FILE = 7, 101, 110
NAN, INF = float("nan"), float("inf")
FLAGS = ((False, False), (True, False), (False, True), (True, True))   # (descending, nulls_first)
_ORDERS = {}


def ks_for(n):
    """k in 1, 2, 63, 64, 65, 256, 257, n - 1, n, n + 1 and 65536"""
    return sorted({k for k in (1, 2, 63, 64, 65, 256, 257, n - 1, n, n + 1, 65536) if 1 <= k <= 65536})


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    capi.load()
    return tmp_path_factory.mktemp("top_k")


class Norm:
    """A table as arrays that compare exactly, whatever reader or writer made them: Timestamps as their int64, a dictionary column
    as its values, floats BY THEIR BITS -- a payload travels bit for bit, a NaN's sign and a zero's included -- with the slots of
    NULLs cleared."""

    def __init__(self, table):
        self.names, self.cols = list(table.column_names), []
        for name in self.names:
            col = table.column(name).combine_chunks()
            if isinstance(col, pa.ChunkedArray):
                col = pa.concat_arrays(col.chunks) if col.num_chunks else pa.array([], col.type)
            if pa.types.is_timestamp(col.type):
                col = col.cast(pa.int64())
            if pa.types.is_dictionary(col.type):
                col = col.cast(col.type.value_type)
            if pa.types.is_floating(col.type):
                bits = np.int64 if col.type == pa.float64() else np.int32
                mask = np.asarray(col.is_null())
                vals = np.asarray(col.fill_null(0.0)).view(bits)
                col = pa.array(vals, mask=mask)
            self.cols.append(col)

    def __eq__(self, other):
        return self.names == other.names and all(a.type == b.type and a.equals(b) for a, b in zip(self.cols, other.cols))

    def __repr__(self):
        return "Norm(%s)" % ", ".join("%s=%s" % (n, c.slice(0, 8).to_pylist()) for n, c in zip(self.names, self.cols))


def norm(table):
    return Norm(table)


def keys_of(by):
    return [(k.column, k.descending, k.nulls_first) for k in by]


def model_order(table, by, kept, tag=None):
    """The model's full order over the kept rows (the first k of it is the answer for every k), computed once per (tag, keys)"""
    key = (tag, tuple(keys_of(by)))
    if tag is None or key not in _ORDERS:
        cols = {k.column: M.key_values(table.column(k.column)) for k in by}
        rows = [{c: cols[c][i] for c in cols} for i in range(table.num_rows)]
        order = M.top_k_order(rows, keys_of(by), table.num_rows, None if kept is None else list(kept))
        if tag is None:
            return order
        _ORDERS[key] = order
    return _ORDERS[key]


def expect(table, names, order):
    return norm(table.select(list(names)).take(pa.array(order, type=pa.int64())))


def builder(src, names, pred=None, selection=None, prefetch=0, dictionary=None):
    b = TA.builder(src, names, pred=pred, selection=selection, prefetch=prefetch, precision="ns")
    if dictionary:
        b = b.with_dictionary_columns(dictionary)
    return b


def check(src, table, names, by, k, pred=None, selection=None, tag=None, dictionary=None, prefetch=0):
    """builder.top_k against the model: the same rows in the same order, every column"""
    kept = AM.kept_mask(table, pred, selection, BATCH) if (pred is not None or selection is not None) else None
    order = model_order(table, by, kept, tag)[:k]
    got = builder(src, names, pred, selection, prefetch, dictionary).top_k(by, k)
    want = expect(table, names, order)
    assert got.num_rows == len(order), (by, k, got.num_rows, len(order))
    if len(order):
        assert norm(got) == want, (keys_of(by), k)


# ---- every key kind alone, asc / desc x nulls first / last, at every size and null share; k rotates through its list ----
@pytest.mark.parametrize("null_frac", TA.NULLS)
@pytest.mark.parametrize("n", SIZES)
def test_every_key_kind_alone(tmpdir, n, null_frac):
    table = TA.make_table(n, null_frac)
    path = TA.pyarrow_file(tmpdir, n, null_frac)
    ks = ks_for(n)
    combos = [(c, f) for c in TA.VALUE_COLS for f in FLAGS]
    if n > 4096:  # (the model's sort of 70 001 rows is what costs: every kind once, the flags rotating)
        combos = [(c, FLAGS[i % 4]) for i, c in enumerate(TA.VALUE_COLS)]
    for i, (c, (desc, nf)) in enumerate(combos):
        check(path, table, TA.ALL_COLS, [SortKey(c, desc, nf)], ks[i % len(ks)], tag=("kinds", n, null_frac))


# ---- three distinct values: the boundary bin holds far more rows than the remainder, the tie rule decides; all equal; all NULL ----
def tie_table(n):
    rng = np.random.default_rng(5 + n)
    return pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "t": pa.array(rng.integers(0, 3, n), pa.int64()),
                     "same": pa.array(np.full(n, 7, dtype=np.int64)), "none": pa.array([None] * n, pa.int64()),
                     "s": pa.array(["row %d" % x for x in range(n)], pa.string())})


@pytest.mark.parametrize("n", SIZES)
def test_every_k_with_ties_all_equal_and_all_null(n):
    table = tie_table(n)
    data, _ = TA.own_file(table)
    for k in ks_for(n):
        for by in ([SortKey("t")], [SortKey("t", True)], [SortKey("same", True, True)], [SortKey("none")], [SortKey("none", True, True), SortKey("t")]):
            check(data, table, table.column_names, by, k, tag=("ties", n))


# ---- floats with NaN, +-inf, +-0.0; int64 and Decimal(38) extremes ----
def special_table(n):
    rng = np.random.default_rng(9)
    f = rng.choice(np.array([NAN, -NAN, INF, -INF, 0.0, -0.0, 1.5, -1.5, 5e-324, -5e-324, 1.7976931348623157e308]), n)
    f32 = rng.choice(np.array([NAN, INF, -INF, 0.0, -0.0, 1.5, -2.5, 3.4028235e38, 1e-45], dtype=np.float32), n)
    i = rng.choice(np.array([-2 ** 63, 2 ** 63 - 1, -1, 0, 1], dtype=np.int64), n)
    big = 10 ** 38 - 1
    d = [D(int(x)) for x in rng.choice(np.array([-big, big, -1, 0, 1, -(2 ** 64), 2 ** 64, -(2 ** 63), 2 ** 63 - 1], dtype=object), n)]

    def nulls(values):
        return [None if m else v for v, m in zip(values, rng.random(n) < 0.1)]
    return pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "f64": pa.array(nulls(f.tolist()), pa.float64()), "f32": pa.array(nulls(f32.tolist()), pa.float32()),
                     "i64": pa.array(nulls(i.tolist()), pa.int64()), "dec38": pa.array(nulls(d), pa.decimal128(38, 0))})


@pytest.mark.parametrize("column", ("f64", "f32", "i64", "dec38"))
def test_float_specials_and_integer_and_decimal_extremes(column):
    n = 2049
    table = special_table(n)
    data, _ = TA.own_file(table)
    for desc, nf in FLAGS:
        for k in (1, 65, 257, n):
            check(data, table, table.column_names, [SortKey(column, desc, nf)], k, tag=("special", n))


# ---- four keys of mixed kinds ----
@pytest.mark.parametrize("n", (1025, 2049, 70_001))
def test_four_keys_of_mixed_kinds(tmpdir, n):
    table = TA.make_table(n, 0.3)
    path = TA.pyarrow_file(tmpdir, n, 0.3)
    by = [SortKey("g"), SortKey("b", True, True), SortKey("i8", False, True), SortKey("dec38", True)]
    for k in (1, 257, min(n, 65536)):
        check(path, table, TA.ALL_COLS, by, k, tag=("four", n))
    if n < 4096:
        check(path, table, TA.ALL_COLS, [SortKey("b"), SortKey("date", True), SortKey("f32"), SortKey("ts", True, True)], 300, tag=("four", n))


# ---- under a row filter, under a row selection, under both, with none ----
@pytest.mark.parametrize("n", (65, 1025, 2049))
def test_under_a_row_filter_a_selection_both_and_none(tmpdir, n):
    table = TA.make_table(n, 0.3)
    path = TA.pyarrow_file(tmpdir, n, 0.3)
    arms = TA.arms(n) + [("selection", None, TA.selection_over(n))]
    for name, pred, sel in arms:
        for by, k in (([SortKey("i32", True)], 65), ([SortKey("g"), SortKey("f64", False, True)], 257), ([SortKey("b", True, True)], n)):
            check(path, table, TA.ALL_COLS, by, k, pred=pred, selection=sel)


# ---- String, Binary and dictionary-output payload columns ----
def test_string_binary_and_dictionary_payload(tmpdir):
    n = 2049
    rng = np.random.default_rng(3)
    words = ["", "a", "bb", "a longer value that does not fit a lane's short copy: " + "x" * 80, "zeta"]
    table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "v": pa.array(rng.integers(-50, 50, n), pa.int64()),
                      "s": pa.array([None if x % 7 == 0 else "row %d %s" % (x, words[x % 5]) for x in range(n)], pa.string()),
                      "bin": pa.array([None if x % 5 == 0 else bytes([x % 256]) * (x % 19) for x in range(n)], pa.binary()),
                      "d": pa.array([None if x % 11 == 0 else words[x % 5] for x in range(n)], pa.string())})
    path = str(tmpdir / "payload.orc")
    orc.write_table(table, path, compression="uncompressed", stripe_size=64 << 20)
    for k in (1, 64, 1025, n + 1):
        check(path, table, table.column_names, [SortKey("v", True)], k, dictionary=["d"], tag="payload")
        check(path, table, table.column_names, [SortKey("v")], k, pred=P.gt("id", V.Int64(100)))


# ---- the same call twice: equal batches ----
def test_the_same_call_twice_gives_equal_batches(tmpdir):
    n = 70_001
    path = TA.pyarrow_file(tmpdir, n, 0.3)
    runs = []
    for _ in range(2):
        r = builder(path, TA.ALL_COLS, pred=P.lt("g", V.Int64(2))).with_top_k([SortKey("g", True), SortKey("f32", False, True)], 1000).build()
        runs.append([b for b in r])
        r.close()
    assert len(runs[0]) == len(runs[1]) == 1
    for a, b in zip(*runs):
        assert norm(pa.Table.from_batches([a])) == norm(pa.Table.from_batches([b]))


# ---- a 3-stripe file through the reader: the stripes' candidates, the order over them, the counters, the bytes ----
def three_stripes():
    n = 3 * 2049
    rng = np.random.default_rng(21)
    table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "t": pa.array(rng.integers(0, 5, n), pa.int64()),
                      "f": pa.array([None if x % 13 == 0 else float(v) for x, v in enumerate(rng.integers(-4, 4, n))], pa.float64()),
                      "s": pa.array(["row %d" % x for x in range(n)], pa.string())})
    data, rows = TA.own_file(table, stripes=3)
    assert rows == [2049, 2049, 2049]
    return table, data


@pytest.mark.parametrize("mode", ("serial", "read-ahead", "device"))
def test_three_stripes_through_the_reader(mode):
    prefetch, device = (2 if mode == "read-ahead" else 0), mode == "device"
    table, data = three_stripes()
    names = table.column_names
    pred = P.gte("t", V.Int64(1))
    kept = AM.kept_mask(table, pred, None, BATCH)
    plain = builder(data, names, pred=pred, prefetch=prefetch).build()
    list(plain)
    d2h_plain = plain.d2h_bytes()
    plain.close()
    for by, k in (([SortKey("t")], 100), ([SortKey("f", True, True), SortKey("t", True)], 1500), ([SortKey("t", True)], 65536)):
        b = builder(data, names, pred=pred, prefetch=prefetch).with_top_k(by, k)
        if device:
            b = b.with_device_output()
        r = b.build()
        with pytest.raises(capi.OrcGpuError) as e:      # before the end of the file
            r.top_k_order()
        assert e.value.code == INVALID and "top-k:" in str(e.value)
        batches = [(x.to_pyarrow() if device else x) for x in r]
        assert all(x.num_rows <= BATCH for x in batches)
        # every stripe hands out at most k rows, its own best in order
        handed = concat_batches(batches)
        ids = handed.column("id").to_pylist()
        for s in range(3):
            mine = [i for i in ids if 2049 * s <= i < 2049 * (s + 1)]
            stripe_kept = np.zeros(len(kept), bool)
            stripe_kept[2049 * s:2049 * (s + 1)] = kept[2049 * s:2049 * (s + 1)]
            assert mine == model_order(table, by, stripe_kept)[:k], (s, by, k)
        order = r.top_k_order()
        want = model_order(table, by, kept)[:k]
        assert len(order) == len(want) == min(k, int(kept.sum()))
        assert norm(handed.take(pa.array(order, type=pa.uint64()))) == expect(table, names, want)   # ties across stripes included
        assert r.filter_rows() == (table.num_rows, int(kept.sum()))
        if not device and k < 2049:
            assert 0 < r.d2h_bytes() < d2h_plain
        n = C.c_uint64(0)
        assert r._ctx.L.orcgpu_reader_top_k_order(r._h, None, 0, C.byref(n)) == INVALID and n.value == len(want)   # cap too small
        r.close()
    # builder.top_k: the same answer as one table
    got = builder(data, names, pred=pred, prefetch=prefetch).top_k([("f", "desc"), "t"], 200)
    assert norm(got) == expect(table, names, model_order(table, [SortKey("f", True), SortKey("t")], kept)[:200])


def test_no_kept_row_gives_no_batch_and_an_empty_order():
    table, data = three_stripes()
    r = builder(data, table.column_names, pred=P.lt("id", V.Int64(-1))).with_top_k("t", 10).build()
    assert list(r) == [] and r.top_k_order() == [] and r.filter_rows() == (table.num_rows, 0)
    r.close()
    assert builder(data, table.column_names, pred=P.lt("id", V.Int64(-1))).top_k("t", 10).num_rows == 0


# ---- orcgpu_result_top_k through the C ABI on a decoded result ----
def result_rows(res):
    out = []
    for b in range(res.n_batches):
        cols = []
        for col in range(2):
            v = res.batch(b, col)
            vals = np.frombuffer(v["values"], dtype=np.int64)[:v["length"]]
            valid = np.unpackbits(np.frombuffer(v["validity"], dtype=np.uint8), bitorder="little")[:v["length"]] if v["validity"] is not None else np.ones(v["length"], np.uint8)
            cols.append([int(x) if p else None for x, p in zip(vals, valid)])
        out += list(zip(*cols))
    return out


@pytest.mark.parametrize("n,k", ((4097, 1), (4097, 300), (4097, 5000), (63, 64)))
def test_result_top_k_through_the_c_abi(n, k):
    c = TA.ctx()
    res, table = TA.stripe_result(n, 1000)
    by = [SortKey("v", True, True), SortKey("id", True)]
    kept, out = c.result_top_k(res, by, k, ["id", "v"])          # n_nodes = 0: no predicate
    order = model_order(table, by, None)[:k]
    assert (kept, out) == (n, len(order)) and res.rows == len(order)
    assert result_rows(res) == [(table.column("id")[i].as_py(), table.column("v")[i].as_py()) for i in order]
    res.free()
    # under a predicate, on a selected result
    res, table = TA.stripe_result(n, 1000)
    sel = [(10, True), (n - 30, False), (20, True)]
    res.select(sel)
    pred = P.gt("v", V.Int64(-10))
    keep = AM.kept_mask(table, pred, sel, 1000)
    kept, out = c.result_top_k(res, [SortKey("v")], k, ["id", "v"], pred)
    order = model_order(table, [SortKey("v")], keep)[:k]
    assert (kept, out) == (int(keep.sum()), len(order))
    assert result_rows(res) == [(table.column("id")[i].as_py(), table.column("v")[i].as_py()) for i in order]
    res.free()


# ---- every refusal, with status and message ----
def refused(b, by, k, code, *words):
    r = b.with_top_k(by, k).build()
    with pytest.raises(capi.OrcGpuError) as e:
        next(r)
    assert e.value.code == code and "top-k:" in str(e.value), str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    with pytest.raises(StopIteration):     # a refusal is final: the iterator has ended
        next(r)
    with pytest.raises(capi.OrcGpuError):
        r.top_k_order()
    r.close()


def test_refusals_are_loud_and_name_the_column(tmpdir):
    path = TA.pyarrow_file(tmpdir, 1025, 0.3)
    refused(builder(path, TA.ALL_COLS), "s", 5, UNSUPPORTED, "'s'", "String")
    refused(builder(path, TA.ALL_COLS, dictionary=["s"]), "s", 5, UNSUPPORTED, "'s'", "dictionary column")
    refused(builder(path, TA.ALL_COLS), ["i64", "nope"], 5, INVALID, "'nope'")
    refused(builder(path, ["id", "g"]), "i64", 5, INVALID, "'i64'")                                  # not projected
    for col in ("ts", "tsi"):                                                                        # Timestamp decoded to Decimal128(38, 9)
        sch = pa.schema([("id", pa.int64()), ("ts", pa.decimal128(38, 9)), ("tsi", pa.decimal128(38, 9))])
        refused(builder(path, ["id", "ts", "tsi"]).with_schema(sch), col, 5, UNSUPPORTED, "'%s'" % col, "Decimal128(38, 9)")
    # a Binary key and a nested column in the result
    t = pa.table({"id": pa.array([1, 2, 3], pa.int64()), "bin": pa.array([b"a", b"b", None], pa.binary()),
                  "st": pa.array([{"x": 1}, {"x": 2}, None], pa.struct([("x", pa.int64())]))})
    p2 = str(tmpdir / "nested.orc")
    orc.write_table(t, p2, compression="uncompressed")
    b = TA.ArrowReaderBuilder.try_new(p2, TA.ctx()).with_prefetch(0)
    refused(b.with_projection(["id", "bin"]), "bin", 2, UNSUPPORTED, "'bin'", "Binary")
    b = TA.ArrowReaderBuilder.try_new(p2, TA.ctx()).with_prefetch(0)
    refused(b, "id", 2, UNSUPPORTED, "'st'", "nested")
    # what the Python checks catch first, at the C ABI: a key twice, no key, five keys, k = 0, k above the limit
    c = TA.ctx()

    def set_top_k(cols, k):
        h = TA.ArrowReaderBuilder.try_new(path, c).with_prefetch(0)
        names = [x.encode() for x in cols]
        arr = (SortKeyStruct * max(1, len(cols)))()
        for i, x in enumerate(names):
            arr[i].column = x
        return c.L.orcgpu_reader_set_top_k(h._h, arr, len(cols), k), h

    for cols, k, words in (([], 5, ("no sort key",)), (["i8", "i16", "i32", "i64", "g"], 5, ("more than",)), (["i8"], 0, ("k must be",)), (["i8"], 65537, ("k must be",))):
        rc, h = set_top_k(cols, k)
        assert rc == INVALID, (cols, k, rc)
        with pytest.raises(capi.OrcGpuError) as e:
            c._check(rc)
        assert "top-k:" in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
    rc, h = set_top_k(["i8", "i64", "i8"], 5)
    assert rc == 0
    r = h.build()
    with pytest.raises(capi.OrcGpuError) as e:
        next(r)
    assert e.value.code == INVALID and "'i8'" in str(e.value) and "listed twice" in str(e.value)
    r.close()
    # the same at orcgpu_result_top_k
    res, _ = TA.stripe_result(100, 1000)
    names = (C.c_char_p * 2)(b"id", b"v")
    arr = (SortKeyStruct * 5)()
    for i in range(5):
        arr[i].column = b"v"
    kept, out = C.c_uint64(7), C.c_uint64(7)
    for n_keys, k in ((0, 5), (5, 5), (1, 0), (1, 65537), (2, 5)):
        assert c.L.orcgpu_result_top_k(c.h, res.h, None, 0, names, 2, arr, n_keys, k, C.byref(kept), C.byref(out)) == INVALID, (n_keys, k)
        assert (kept.value, out.value) == (0, 0)
    assert res.rows == 100                                                                           # nothing changed
    res.free()


def test_top_k_with_aggregates_is_refused_at_the_second_setter_and_the_reader_stays_usable(tmpdir):
    from orc_rust_amd.aggregate import Agg
    n = 1025
    table = TA.make_table(n, 0.3)
    path = TA.pyarrow_file(tmpdir, n, 0.3)
    # top-k first: the aggregates are refused, the top-k still runs
    b = builder(path, TA.ALL_COLS).with_top_k("i32", 10)
    with pytest.raises(capi.OrcGpuError) as e:
        b.aggregating_reader([Agg.count_rows()])
    assert e.value.code == INVALID
    r = b.build()
    got = concat_batches(list(r))
    assert norm(got.take(pa.array(r.top_k_order(), type=pa.uint64()))) == expect(table, TA.ALL_COLS, model_order(table, [SortKey("i32")], None)[:10])
    r.close()
    # aggregates first: the top-k is refused, the aggregation still runs
    from orc_rust_amd import aggregate as A
    b = builder(path, TA.ALL_COLS)
    arr, keep = A.spec_array([Agg.count_rows()])
    b._ctx._check(b._ctx.L.orcgpu_reader_set_aggregates(b._h, arr, len(arr)))
    with pytest.raises(capi.OrcGpuError) as e:
        b.with_top_k("i32", 10)
    assert e.value.code == INVALID and "top-k:" in str(e.value)
    r = b.build()
    r._agg_specs = [Agg.count_rows()]
    assert r.aggregate() == [n]
    with pytest.raises(capi.OrcGpuError):      # a reader without top-k
        r.top_k_order()
    r.close()
