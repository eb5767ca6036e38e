"""GROUP BY for the GPU aggregates (orcgpu_result_aggregate_groups, orcgpu_reader_set_group_by / orcgpu_reader_aggregate_groups:
device/agg_group_kernels.hip) against the model of tests/group_model.py.  Files are written with pyarrow.orc and with this
project's writer, as tests/test_gpu_aggregate.py does (whose tables, writers and value check are used here); the expected groups
and values come from the table that was written, through the model, never from a read of the file.  Batch size 1024."""
import ctypes as C
import decimal
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import agg_model as AM
import group_model as GM
import selection_model as SM
import test_gpu_aggregate as TA
from orc_rust_amd import aggregate as A
from orc_rust_amd import capi, gen
from orc_rust_amd.aggregate import Agg
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

pytestmark = pytest.mark.gpu

D = decimal.Decimal
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = TA.BATCH
MISMATCHED, UNSUPPORTED, INVALID = 6, 7, 101
FLAGS = ["A", "N", "R", None]
SMALL_SPECS_COLS = ("i64", "f64", "dec")
_KEYED = {}


def keyed_table(n, null_frac=0.3, date=False):
    """TA.make_table(n, null_frac) with key columns in front of it: `flag` and `status` cycle so that every word of the mask holds
    every group (Q1's two String keys, one with NULLs); `half` has two groups; `k64` 64 distinct values in every word"""
    key = (n, null_frac, date)
    if key not in _KEYED:
        t = TA.make_table(n, null_frac)
        if not date:
            t = t.drop_columns(["date"])
        ids = np.arange(n)
        t = t.append_column("flag", pa.array([FLAGS[(x * 7) % 4] for x in ids], pa.string()))
        t = t.append_column("status", pa.array(["O" if (x // 3) % 2 else "F" for x in ids], pa.string()))
        t = t.append_column("half", pa.array((ids % 2).astype(np.int8), pa.int8()))
        t = t.append_column("k64", pa.array(((ids * 5) % 64).astype(np.int32), pa.int32()))
        _KEYED[key] = t
    return _KEYED[key]


def drain(reader, specs):
    """([(keys, values)], (rows seen, rows kept), bytes copied back) of a grouped reader; a set overflow flag becomes AM.OVERFLOW"""
    try:
        raw = reader.aggregate(raw=True)
        got = [(keys, [AM.OVERFLOW if v.overflow else A.value_of(v, s) for v, s in zip(vals, specs)]) for keys, vals in raw]
        return got, reader.filter_rows(), reader.d2h_bytes()
    finally:
        reader.close()


def run(src, names, specs, group_by, **kw):
    return drain(TA.builder(src, names, **kw).aggregating_reader(specs, group_by=group_by), specs)


def check_groups(table, specs, group_by, got, keep, what, ts_unit="ns"):
    want = GM.group_rows(table, group_by, keep, ts_unit)
    assert [tuple(GM.key_id(k) for k in keys) for keys, _ in got] == [tuple(GM.key_id(k) for k in keys) for keys, _ in want], (what, [k for k, _ in got][:8], [k for k, _ in want][:8])
    for (keys, vals), (_, mask) in zip(got, want):      # (per group its rows as a table of their own: the model then costs the table once)
        sub = table.filter(pa.array(mask))
        TA.check(sub, specs, vals, np.ones(sub.num_rows, bool), (what, keys), ts_unit=ts_unit)


def refused(call, code, *words):
    with pytest.raises(capi.OrcGpuError) as e:
        call()
    assert e.value.code == code and all(w in str(e.value) for w in words), (code, words, str(e.value))


# ---- rows: across a word of the mask, a batch, a block's share and several blocks ----
@pytest.mark.parametrize("n", TA.SIZES)
def test_every_size_and_arm(n):
    table = keyed_table(n)
    names = ["id", "g", "flag", "status", "half"] + [c for c in TA.VALUE_COLS if c != "date"]
    arms = TA.arms(n)
    if n > 1025:        # (the model is plain Python: the larger sizes take the columns of one kind each, the largest two arms)
        names = ["id", "g", "flag", "status", "half"] + list(SMALL_SPECS_COLS)
    if n > 2049:
        arms = [arms[0], arms[4]]
    data, _ = TA.own_file(table.select(names))
    specs = TA.specs_for(names)
    for name, pred, sel in arms:
        if n == 0 and sel is not None:
            sel = [(5, True), (5, False)]
        keep = AM.kept_mask(table, pred, sel, BATCH)
        for group_by in (["flag", "status"], ["half"]):
            got, (seen, kept), d2h = run(data, names, specs, group_by, pred=pred, selection=sel)
            check_groups(table, specs, group_by, got, keep, (n, name, group_by))
            assert d2h == 0
            assert (seen, kept) == (int(AM.kept_mask(table, None, sel, BATCH).sum()), int(keep.sum())), (name, seen, kept)
        if not keep.any():
            assert got == []                # no kept row: zero groups, not one group of NULLs


# ---- groups: 1, 2, 64 in one word, 255, 256, and 257 refused ----
@pytest.mark.parametrize("n_groups", (1, 2, 64, 255, 256))
def test_group_counts(n_groups):
    n = 1025
    base = TA.make_table(n, 0.3)
    ids = np.arange(n)
    k = (ids * 3) % n_groups if n_groups <= 64 else ids % n_groups      # 64: every word holds 64 distinct groups
    table = base.select(["id", "i64", "f64", "dec"]).append_column("k", pa.array(k.astype(np.int64) - 7, pa.int64()))
    if n_groups == 64:
        assert len(set(k[:64])) == 64 and len(set(k[64:128])) == 64
    data, _ = TA.own_file(table)
    specs = TA.specs_for(["i64", "f64", "dec"])
    got, _, _ = run(data, table.column_names, specs, ["k"])
    assert len(got) == n_groups
    check_groups(table, specs, ["k"], got, np.ones(n, bool), n_groups)
    pred = P.lt("id", V.Int64(600))
    got, _, _ = run(data, table.column_names, specs, ["k"], pred=pred)
    check_groups(table, specs, ["k"], got, AM.kept_mask(table, pred), (n_groups, "filtered"))


def test_257_groups_are_refused_with_the_limit():
    n = 1025
    table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "k": pa.array((np.arange(n) % 257).astype(np.int64))})
    data, _ = TA.own_file(table)
    specs = [Agg.count_rows()]
    for prefetch in (0, 2):
        r = TA.builder(data, ["id", "k"], prefetch=prefetch).aggregating_reader(specs, group_by=["k"])
        refused(r.aggregate, UNSUPPORTED, "256")
        r.close()
    got, _, _ = run(data, ["id", "k"], specs, ["k"], pred=P.lt("id", V.Int64(256)))       # the 257th group only among dropped rows
    assert [k for k, _ in got] == [(x,) for x in range(256)] and all(v == [1] for _, v in got)
    # every row a group of its own, far past the limit: refused all the same, nothing written out of bounds
    big = pa.table({"id": pa.array(np.arange(5000, dtype=np.int64))})
    data, _ = TA.own_file(big)
    r = TA.builder(data, ["id"]).aggregating_reader(specs, group_by=["id"])
    refused(r.aggregate, UNSUPPORTED, "256")
    r.close()


# ---- keys: every kind alone, at null fractions 0, 0.3 and 1.0 ----
KEY_KINDS = ("ki8", "ki16", "ki32", "ki64", "kdate", "kb", "kts", "ktsi", "kdec", "kdec38", "ks")


def kinds_table(n, null_frac):
    rng = np.random.default_rng(5)
    pick = rng.integers(0, 5, n)

    def nulls(values):
        mask = rng.random(n) < null_frac if null_frac < 1.0 else np.ones(n, bool)
        return [None if m else v for v, m in zip(values, mask)]

    def of(choices):
        return [choices[p] for p in pick]

    base = TA.make_table(n, 0.3)
    big = 10 ** 37
    cols = {
        "id": base.column("id"), "i64": base.column("i64"), "f64": base.column("f64"), "dec": base.column("dec"),
        "ki8": pa.array(nulls(of([-128, -1, 0, 1, 127])), pa.int8()),
        "ki16": pa.array(nulls(of([-2 ** 15, -1, 0, 1, 2 ** 15 - 1])), pa.int16()),
        "ki32": pa.array(nulls(of([-2 ** 31, -1, 0, 1, 2 ** 31 - 1])), pa.int32()),
        "ki64": pa.array(nulls(of([-2 ** 63, -1, 0, 2 ** 32, 2 ** 63 - 1])), pa.int64()),
        "kdate": pa.array(nulls(of([-20000, -1, 0, 1, 20000])), pa.date32()),
        "kb": pa.array(nulls([bool(p & 1) for p in pick]), pa.bool_()),
        "kts": pa.array(nulls(of([TA.T0, TA.T0 + 1000, TA.T0 + 10 ** 12, 1000, 2000])), pa.timestamp("ns")),
        "ktsi": pa.array(nulls(of([TA.T0, TA.T0 + 1000, TA.T0 + 10 ** 12, 1000, 2000])), pa.timestamp("ns", tz="UTC")),
        "kdec": pa.array(nulls(of([D("-1.50"), D("0.00"), D("1.50"), D("0.01"), D("-0.01")])), pa.decimal128(15, 2)),
        "kdec38": pa.array(nulls(of([D(-big * 9), D(-1), D(0), D(2 ** 64), D(big * 9)])), pa.decimal128(38, 0)),   # (the low word alone does not tell them apart)
        "ks": pa.array(nulls(of(["", "a", "ab", "a ", "né"])), pa.string()),
    }
    return pa.table(cols)


@pytest.mark.parametrize("null_frac", TA.NULLS)
def test_every_key_kind(tmp_path, null_frac):
    capi.load()
    n = 1025
    table = kinds_table(n, null_frac)
    path = str(tmp_path / "kinds.orc")
    orc.write_table(table, path, compression="uncompressed", stripe_size=64 << 20)
    specs = [Agg.count_rows(), Agg.count("i64"), Agg.sum("i64"), Agg.min("dec"), Agg.max("f64"), Agg.sum("dec")]
    keep = np.ones(n, bool)
    for key in KEY_KINDS:
        names = ["id", "i64", "f64", "dec", key]
        got, _, d2h = run(path, names, specs + [Agg.count(key)], [key])
        check_groups(table, specs + [Agg.count(key)], [key], got, keep, (key, null_frac))
        assert d2h == 0
        if null_frac == 1.0:
            assert got[0][0] == (None,) and len(got) == 1 and got[0][1][0] == n      # one group, the NULL key
        if key in ("kts", "ktsi"):
            assert all(k[0] is None or k[0].units == "ns" for k, _ in got)
    # a Timestamp key in microseconds, and the own writer's file of the same table (no Date column there)
    got, _, _ = run(path, ["id", "i64", "f64", "dec", "kts"], specs, ["kts"], precision="us")
    check_groups(table, specs, ["kts"], got, keep, "us", ts_unit="us")
    assert all(k[0] is None or k[0].units == "us" for k, _ in got)
    data, _ = TA.own_file(table.drop_columns(["kdate"]))
    for key in ("ki8", "kb", "kdec38", "ks", "ktsi"):
        got, _, _ = run(data, ["id", "i64", "f64", "dec", key], specs, [key], pred=P.gte("id", V.Int64(100)))
        check_groups(table, specs, [key], got, AM.kept_mask(table, P.gte("id", V.Int64(100))), ("own", key, null_frac))


def test_mixed_keys_two_to_four():
    n = 2049
    table = kinds_table(n, 0.3).drop_columns(["kdate"])
    data, _ = TA.own_file(table)
    specs = TA.specs_for(["i64", "f64", "dec"])
    pred = P.gt("i64", V.Int64(0))
    for group_by in (["ks", "kb"], ["ki32", "kdec", "kb", "ks"], ["kts", "ki8", "kdec38"], ["kb", "ki64"]):
        names = ["id", "i64", "f64", "dec"] + group_by
        for p in (None, pred):
            got, _, _ = run(data, names, specs, group_by, pred=p)
            check_groups(table, specs, group_by, got, AM.kept_mask(table, p), (group_by, p is not None))
        assert len(got) > 4
    # a key column may be an aggregated column too
    got, _, _ = run(data, ["id", "ki64", "kdec"], [Agg.sum("ki64"), Agg.min("kdec"), Agg.count("ki64")], ["ki64", "kdec"])
    check_groups(table, [Agg.sum("ki64"), Agg.min("kdec"), Agg.count("ki64")], ["ki64", "kdec"], got, np.ones(n, bool), "key and value")


def test_zero_null_and_the_empty_string_are_distinct_groups():
    i = [0, None, 0, None, 0, None] * 30
    s = ["", "", None, None, "0", "0"] * 30
    b = [False, None, False, True, None, True] * 30
    table = pa.table({"id": pa.array(np.arange(180, dtype=np.int64)), "i": pa.array(i, pa.int64()), "s": pa.array(s, pa.string()), "b": pa.array(b, pa.bool_())})
    data, _ = TA.own_file(table)
    got, _, _ = run(data, table.column_names, [Agg.count_rows()], ["i", "s"])
    assert got == [((0, ""), [30]), ((None, ""), [30]), ((0, None), [30]), ((None, None), [30]), ((0, "0"), [30]), ((None, "0"), [30])]
    got, _, _ = run(data, table.column_names, [Agg.count_rows()], ["b"])
    assert got == [((False,), [60]), ((None,), [60]), ((True,), [60])] and got[0][0][0] is False
    got, _, _ = run(data, table.column_names, [Agg.count_rows(), Agg.sum("id")], ["s"])
    check_groups(table, [Agg.count_rows(), Agg.sum("id")], ["s"], got, np.ones(180, bool), "s")


def char_stripe(n=1100, batch=1000):
    """a hand-staged stripe with a Char(4) column whose values carry their padding, and a String column with the same text unpadded"""
    texts = ["a", "ab", "a b", "abcd", ""]
    plain = [texts[(x * 3) % 5] for x in range(n)]
    padded = [(t + "    ")[:4] for t in plain]
    ids = np.arange(n, dtype=np.int64)
    cols = [{"column_id": 1, "orc_type": 4, "encoding": 2}, {"column_id": 2, "orc_type": 7, "encoding": 2}, {"column_id": 3, "orc_type": 17, "encoding": 2}]
    streams = [(1, 1, gen.rle2(ids, signed=True)),
               (2, 1, "".join(plain).encode()), (2, 2, gen.rle2(np.array([len(x) for x in plain], dtype=np.int64), signed=False)),
               (3, 1, "".join(padded).encode()), (3, 2, gen.rle2(np.array([len(x) for x in padded], dtype=np.int64), signed=False))]
    c = TA.ctx()
    staged = c.stage(n, streams, cols, batch_size=batch)
    res = c.decode([staged])[0]
    staged.free()
    return res, pa.table({"id": pa.array(ids), "s": pa.array(plain), "c4": pa.array(padded)})


def test_char_keys_keep_their_padding():
    res, table = char_stripe()
    c = TA.ctx()
    specs = [Agg.count_rows(), Agg.sum("id")]
    got = c.result_aggregate_groups(res, specs, ["c4"], ["id", "s", "c4"])
    assert [k for k, _ in got] == [("a   ",), ("abcd",), ("ab  ",), ("    ",), ("a b ",)]
    assert got == GM.aggregate_groups(table, specs, ["c4"])
    assert c.result_aggregate_groups(res, specs, ["s", "c4"], ["id", "s", "c4"]) == GM.aggregate_groups(table, specs, ["s", "c4"])
    res.free()


def test_string_keys_of_64_and_65_bytes():
    n = 300
    s = [("x%02d" % (k % 3)) + "y" * 61 for k in range(n)]          # 64 bytes each
    s[200] = "z" * 65
    table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "s": pa.array(s, pa.string()), "t": pa.array(["é" * 32] * n, pa.string())})
    data, _ = TA.own_file(table)
    specs = [Agg.count_rows(), Agg.sum("id")]
    drop = P.ne("id", V.Int64(200))
    got, _, _ = run(data, table.column_names, specs, ["s", "t"], pred=drop)             # 64 bytes pass; the 65 only in a dropped row
    assert got == GM.aggregate_groups(table, specs, ["s", "t"], drop) and len(got) == 3 and all(len(k[0].encode()) == 64 == len(k[1].encode()) for k, _ in got)
    assert GM.aggregate_groups(table, specs, ["s"]) == GM.KEY_TOO_LONG
    for group_by in (["s"], ["t", "s"]):
        r = TA.builder(data, table.column_names).aggregating_reader(specs, group_by=group_by)
        refused(r.aggregate, UNSUPPORTED, "'s'", "64")
        r.close()


# ---- values ----
def test_float_sums_within_the_bound_and_bit_identical():
    n = 70_001
    rng = np.random.default_rng(8)
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)).tolist()      # sixteen orders of magnitude: the order of summation shows
    table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "x": pa.array(x, pa.float64()),
                      "y": pa.array(rng.standard_normal(n).astype(np.float32).tolist(), pa.float32()),
                      "flag": pa.array([FLAGS[int(v)] for v in rng.integers(0, 4, n)], pa.string()), "k": pa.array(rng.integers(0, 40, n), pa.int64())})
    data, _ = TA.own_file(table)
    specs = [Agg.sum("x"), Agg.sum("y"), Agg.sum_product("x", "y")]
    for group_by in (["flag"], ["k"]):                  # few groups in a word (the tree path) and many (the rounds path)
        runs = [TA.builder(data, table.column_names).aggregate(specs, raw=True, group_by=group_by) for _ in range(2)]
        check_groups(table, specs, group_by, [(k, [v.f for v in vals]) for k, vals in runs[0]], np.ones(n, bool), group_by)
        bits = [[(k, [struct.pack("<d", v.f) for v in vals]) for k, vals in r] for r in runs]
        assert bits[0] == bits[1]                       # the same 8 bytes


def test_an_overflow_stays_in_its_group():
    n = 1025
    vals = [D(10 ** 38 - 1 - (n - 2))] + [D(1)] * (n - 1)
    k = [1] * (n - 1) + [2]                     # group 1: 10^38 - 1, fits; with the last row it would not
    table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "k": pa.array(k, pa.int64()), "d": pa.array(vals, pa.decimal128(38, 0))})
    data, _ = TA.own_file(table)
    specs = [Agg.sum("d"), Agg.count_rows()]
    got, _, _ = run(data, table.column_names, specs, ["k"])
    assert got == [((1,), [D(10 ** 38 - 1), n - 1]), ((2,), [D(1), 1])]
    table2 = table.set_column(1, "k", pa.array([1] * (n - 3) + [2, 2, 1], pa.int64()))       # now group 1 reaches 10^38 - 1: still fits ...
    table3 = table.set_column(1, "k", pa.array([1] * (n - 2) + [2, 1], pa.int64())).set_column(2, "d", pa.array(vals[:-1] + [D(2)], pa.decimal128(38, 0)))
    for t in (table2, table3):                   # ... and in table3 it passes 10^38 next to a group that does not
        data, _ = TA.own_file(t)
        got, _, _ = run(data, t.column_names, specs, ["k"])
        assert got == GM.aggregate_groups(t, specs, ["k"])
    assert got[0][1][0] == AM.OVERFLOW and got[1] == ((2,), [D(1), 1])
    with pytest.raises(OverflowError) as e:
        TA.builder(data, t.column_names).aggregate(specs, group_by=["k"])
    assert "sum('d')" in str(e.value) and "(1,)" in str(e.value)


# ---- paths ----
def test_result_aggregate_groups_on_uniform_selected_and_filtered_results():
    n, batch = 4097, 1000
    c = TA.ctx()
    specs = [Agg.count_rows(), Agg.count("v"), Agg.sum("v"), Agg.min("v"), Agg.max("v"), Agg.sum_product("v", "id")]
    names = ["id", "v"]
    pred = P.and_([P.gt("v", V.Int64(10)), P.gte("id", V.Int64(64))])
    res, table = TA.stripe_result(n, batch)
    before = TA.batches_of(res)
    assert c.result_aggregate_groups(res, specs, ["v"], names) == GM.aggregate_groups(table, specs, ["v"])        # ~100 groups and the NULL key
    assert c.result_aggregate_groups(res, specs, ["v"], names, pred) == GM.aggregate_groups(table, specs, ["v"], pred)
    assert c.result_aggregate_groups(res, specs, ["v"], names, pred) == GM.aggregate_groups(table, specs, ["v"], pred)        # any number of times
    assert TA.batches_of(res) == before
    sel = [(100, True), (900, False), (1000, True), (700, False)]
    res.select(sel)
    keep = np.zeros(n, bool)
    for s, k in SM.stripe_batches(SM.normalise(sel), n, batch):
        keep[s:s + k] = True
    assert c.result_aggregate_groups(res, specs, ["v"], names) == GM.aggregate_groups(table, specs, ["v"], keep=keep)
    keep_f = keep & AM.kept_mask(table, pred)
    assert c.result_aggregate_groups(res, specs, ["v"], names, pred) == GM.aggregate_groups(table, specs, ["v"], keep=keep_f)
    assert c.result_filter(res, pred, names) == int(keep_f.sum())
    assert c.result_aggregate_groups(res, specs, ["v"], names) == GM.aggregate_groups(table, specs, ["v"], keep=keep_f)        # the rows it now holds
    assert c.result_aggregate(res, specs, names) == AM.aggregate(table, specs, keep=keep_f)                                  # the ungrouped call is as it was
    res.free()
    res, table = TA.stripe_result(n, batch)
    nulls = P.or_([P.is_null("v"), P.lt("v", V.Int64(-40))])
    c.result_filter(res, nulls, names)
    assert c.result_aggregate_groups(res, specs, ["v"], names) == GM.aggregate_groups(table, specs, ["v"], nulls)
    res.free()


def stripes_table():
    """three stripes of about equal rows: the group 'late' first appears in stripe 2, 'last' only in stripe 3, and stripe 2
    meets 'b' before 'a'"""
    n = 3 * 1025 + 7
    table = TA.make_table(n, 0.3).drop_columns(["date"])
    k = []
    for x in range(n):
        stripe = min(2, x * 3 // n)
        k.append([["a", "b", None], ["b", "late", "a"], ["last", "a", "late", None]][stripe][x % (3 if stripe < 2 else 4)])
    return table.append_column("k", pa.array(k, pa.string()))


def test_reader_paths_and_order_across_stripes():
    table = stripes_table()
    data, rows = TA.own_file(table, stripes=3)
    assert orc.ORCFile(io.BytesIO(data)).nstripes == 3
    names = ["id", "g", "i64", "f64", "dec", "k"]
    specs = TA.specs_for(names)
    n = table.num_rows
    pred = P.lt("g", V.Int64(1))
    sel = TA.selection_over(n)
    for prefetch in (0, 2):
        for p, s in ((None, None), (pred, None), (None, sel), (pred, sel)):
            keep = AM.kept_mask(table, p, s, BATCH)
            got, (seen, kept), d2h = run(data, names, specs, ["k"], pred=p, selection=s, prefetch=prefetch)
            # the order: stripe by stripe, and within a stripe by first kept row
            parts, at = [], 0
            for r in rows:
                part_keep = np.zeros(n, bool)
                part_keep[at:at + r] = keep[at:at + r]
                parts.append(GM.group_rows(table, ["k"], part_keep))
                at += r
            assert [k for k, _ in got] == GM.merge_stripes(parts), (prefetch, p is not None, s is not None)
            if p is None and s is None:
                assert [k for k, _ in got] == [("a",), ("b",), (None,), ("late",), ("last",)]
            # the values: those of the whole table's groups, whatever their order there
            want = {GM.key_id(k[0]): m for k, m in GM.group_rows(table, ["k"], keep)}
            for keys, vals in got:
                mask = want[GM.key_id(keys[0])]
                exact = [(sp, v) for sp, v in zip(specs, vals) if not isinstance(v, float)]      # (float sums merge in stripe order: other bits)
                assert [v for _, v in exact] == [AM.aggregate_one(table, sp, mask) for sp, _ in exact], keys
                TA.check(table, specs, vals, mask, keys)
            assert d2h == 0
            assert (seen, kept) == (int(AM.kept_mask(table, None, s, BATCH).sum()), int(keep.sum()))


def test_misuse_leaves_the_reader_usable():
    table = stripes_table()
    data, _ = TA.own_file(table, stripes=3)
    specs = [Agg.count_rows(), Agg.sum("i64")]
    c = TA.ctx()
    r = TA.builder(data, ["id", "i64", "k"]).aggregating_reader(specs, group_by=["k"])
    out = (A.AggValue * 2)()
    assert c.L.orcgpu_reader_aggregate(r._h, out) == INVALID        # the ungrouped drain on a grouped reader
    with pytest.raises(capi.OrcGpuError) as e:
        next(r)
    assert e.value.code == INVALID
    got = r.aggregate()                                             # ... and the reader is as usable as before
    assert [k for k, _ in got] == [("a",), ("b",), (None,), ("late",), ("last",)]
    assert sorted(got, key=repr) == sorted(GM.aggregate_groups(table, specs, ["k"]), key=repr)
    with pytest.raises(StopIteration):      # drained: ORCGPU_END_OF_FILE
        r.aggregate()
    handle = C.c_void_p()
    assert c.L.orcgpu_reader_aggregate_groups(r._h, C.byref(handle)) == 110 and not handle.value
    r.close()
    r = TA.builder(data, ["id", "i64", "k"]).aggregating_reader(specs)       # no group-by set
    assert c.L.orcgpu_reader_aggregate_groups(r._h, C.byref(handle)) == INVALID and not handle.value
    assert r.aggregate() == AM.aggregate(table, specs)                       # ... and it aggregates as it always did
    r.close()
    b = TA.builder(data, ["id", "i64", "k"])                                 # a group-by without aggregates: at the drain
    keys = A.key_array(["k"])
    assert c.L.orcgpu_reader_set_group_by(b._h, keys, 1) == 0
    assert c.L.orcgpu_reader_set_group_by(b._h, keys, 0) == INVALID and c.L.orcgpu_reader_set_group_by(b._h, keys, 5) == INVALID
    r = b.build()
    assert c.L.orcgpu_reader_aggregate_groups(r._h, C.byref(handle)) == INVALID and not handle.value
    r.close()


def test_every_refusal_of_the_key_table(tmp_path):
    capi.load()
    n = 1025
    table = kinds_table(n, 0.3)
    table = table.append_column("f32", TA.make_table(n, 0.3).column("f32")).append_column("bin", pa.array([b"x"] * n, pa.binary()))
    path = str(tmp_path / "refusals.orc")
    orc.write_table(table, path, compression="uncompressed", stripe_size=64 << 20)
    names = table.column_names
    specs = [Agg.count_rows()]

    def drain_of(b, group_by):
        r = b.aggregating_reader(specs, group_by=group_by)
        try:
            return r.aggregate()
        finally:
            r.close()

    for col in ("f32", "f64", "bin"):
        refused(lambda: drain_of(TA.builder(path, names), [col]), MISMATCHED, "'%s'" % col)
        refused(lambda: drain_of(TA.builder(path, names), ["ki8", col]), MISMATCHED, "'%s'" % col)
    refused(lambda: drain_of(TA.builder(path, names).with_dictionary_columns(["ks"]), ["ks"]), UNSUPPORTED, "'ks'")
    sch = pa.schema([("id", pa.int64()), ("kts", pa.decimal128(38, 9))])
    refused(lambda: drain_of(TA.builder(path, ["id", "kts"]).with_schema(sch), ["kts"]), UNSUPPORTED, "'kts'")
    refused(lambda: drain_of(TA.builder(path, names), ["nope"]), INVALID, "'nope'")
    refused(lambda: drain_of(TA.builder(path, ["id", "ki8"]), ["ki64"]), INVALID, "'ki64'")        # not projected
    st = pa.table({"id": pa.array([1, 2], pa.int64()), "st": pa.array([{"a": 1}, {"a": 2}], pa.struct([("a", pa.int64())]))})
    data, _ = TA.own_file(st)
    refused(lambda: drain_of(TA.builder(data, ["id", "st"]), ["id"]), UNSUPPORTED, "'st'")
    # what Python refuses first, through the C ABI itself: a key twice, none, five; and orcgpu_result_aggregate_groups' own
    res, _ = TA.stripe_result(100)
    c = TA.ctx()
    cols = (C.c_char_p * 2)(b"id", b"v")
    arr, _keep = A.spec_array(specs)
    out = C.c_void_p()

    def call(keys):
        karr = (C.c_char_p * max(1, len(keys)))(*keys)
        rc = c.L.orcgpu_result_aggregate_groups(c.h, res.h, None, 0, cols, 2, karr, len(keys), arr, 1, C.byref(out))
        assert rc == 0 or not out.value
        return rc, c.L.orcgpu_last_error(c.h).decode() if rc else ""

    rc, msg = call([b"v", b"id", b"v"])
    assert rc == INVALID and "'v'" in msg and "twice" in msg
    assert call([])[0] == INVALID and call([b"id"] * 5)[0] == INVALID
    rc, msg = call([b"w"])
    assert rc == INVALID and "'w'" in msg
    assert c.L.orcgpu_result_aggregate_groups(c.h, res.h, None, 0, cols, 2, (C.c_char_p * 1)(b"v"), 1, arr, 0, C.byref(out)) == INVALID      # no spec
    rc, _ = call([b"v"])
    assert rc == 0 and c.L.orcgpu_groups_count(out) > 1
    key, val = A.GroupKey(), A.AggValue()
    n_groups = c.L.orcgpu_groups_count(out)
    assert c.L.orcgpu_groups_key(out, n_groups, 0, C.byref(key)) == INVALID and c.L.orcgpu_groups_key(out, 0, 1, C.byref(key)) == INVALID
    assert c.L.orcgpu_groups_value(out, 0, 1, C.byref(val)) == INVALID and c.L.orcgpu_groups_value(out, 0, 0, C.byref(val)) == 0
    c.L.orcgpu_groups_free(out)
    res.free()


def test_the_order_of_groups_is_the_same_on_every_run():
    n = 70_001
    rng = np.random.default_rng(12)
    k = rng.integers(0, 48, n)
    k[:48] = rng.permutation(48)                 # every group first appears within the first word: where slot races are likeliest
    table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "k": pa.array(k, pa.int64()), "s": pa.array(["s%d" % (x % 5) for x in k], pa.string()),
                      "x": pa.array(rng.standard_normal(n).tolist(), pa.float64())})
    data, _ = TA.own_file(table)
    specs = [Agg.count_rows(), Agg.sum("x"), Agg.min("id")]
    runs = []
    for _ in range(5):
        raw = TA.builder(data, table.column_names).aggregate(specs, raw=True, group_by=["k", "s"])
        runs.append([(keys, [(v.kind, v.is_null, tuple(v.w), struct.pack("<d", v.f)) for v in vals]) for keys, vals in raw])
    assert all(r == runs[0] for r in runs[1:])
    assert [keys[0] for keys, _ in runs[0]] == [int(x) for x in k[:48]]
    assert [vals[2][2][0] for _, vals in runs[0]] == list(range(48))            # MIN(id) of group g is its first row


# ---- knobs: each in a fresh child process ----
CHILD = r'''
import hashlib, io, os, sys
sys.path.insert(0, %r)
import numpy as np, pyarrow as pa
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.arrow_writer import ArrowWriterBuilder
n = 5000
rng = np.random.default_rng(3)
k = rng.integers(0, 250, n)
table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "k": pa.array(k, pa.int64()),
                  "s": pa.array(["v%%d" %% (x %% 7) for x in k], pa.string()), "x": pa.array(rng.standard_normal(n).tolist(), pa.float64())})
ctx = capi.Context()
out = io.BytesIO()
w = ArrowWriterBuilder(out, table.schema, ctx=ctx).try_build()
for part in (table.slice(0, 2500), table.slice(2500)):      # two stripes
    for batch in part.to_batches():
        w.write(batch)
    w.flush_stripe()
w.close()
w.free()
data = out.getvalue()
specs = [Agg.count_rows(), Agg.sum("x"), Agg.sum("id"), Agg.max("id")]
h = hashlib.sha256()
for group_by in (["k"], ["s", "k"], ["s"]):
    for prefetch in (0, 2):
        for _ in range(2):      # (the second call reuses the workspace: what POISON is about)
            b = ArrowReaderBuilder.try_new(data, ctx).with_batch_size(1024).with_prefetch(prefetch).with_projection(table.column_names)
            got = b.aggregate(specs, group_by=group_by)
            h.update(repr([(k, [v.hex() if isinstance(v, float) else v for v in vals]) for k, vals in got]).encode())
print("GROUPS", len(got), "DIGEST", h.hexdigest())
''' % (ROOT,)


def digest(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ORCGPU_")}
    env.update(extra)
    p = subprocess.run([sys.executable, "-c", CHILD], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return [line for line in p.stdout.decode().splitlines() if line.startswith("GROUPS")][-1]


def test_hash_bits_and_poison_do_not_change_the_answer():
    plain = digest({})          # (a child that faults or times out fails the assert in digest(): no further child is started)
    assert plain.startswith("GROUPS 7 ")
    assert digest({"ORCGPU_GROUP_HASH_BITS": "1"}) == plain       # two hash values for up to 250 keys: probe sequences of ~128
    assert digest({"ORCGPU_POISON": "0xA5"}) == plain
