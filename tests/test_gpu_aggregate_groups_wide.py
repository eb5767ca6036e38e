"""GROUP BY past 256 groups a stripe: the wide path (device/agg_group_wide_kernels.hip), taken when max_groups is set above 256
(orcgpu_reader_set_group_limits, orcgpu_result_aggregate_groups_limit).  Files are written with this project's writer and with
pyarrow.orc, batch size 1024; the expected groups and values come from the table that was written, never from a read.  For ALL
groups: the order, COUNT_ROWS and the integer SUM / MIN / MAX of `id` against numpy; for a seeded sample of at most 32 groups plus
the first and the last: every aggregate against the models of tests/agg_model.py and tests/agg_expr_model.py; Double sums bit for
bit against tests/group_wide_model.py."""
import io
import os
import struct
import subprocess
import sys

import decimal
import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import agg_model as AM
import group_model as GM
import group_wide_model as WM
import test_gpu_aggregate as TA
import test_gpu_aggregate_expr as TX
import test_gpu_aggregate_groups as TG
from orc_rust_amd import aggregate as A
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg, col
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

pytestmark = pytest.mark.gpu

D = decimal.Decimal
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = TA.BATCH
UNSUPPORTED = 7
ID_SPECS = [Agg.count_rows(), Agg.sum("id"), Agg.min("id"), Agg.max("id")]     # what is checked for ALL groups


def run(src, names, specs, group_by, max_groups, max_total=None, **kw):
    return TG.drain(TA.builder(src, names, **kw).aggregating_reader(specs, group_by=group_by, max_groups=max_groups, max_total_groups=max_total), specs)


def int_table(k, n_extra=True):
    """id, the int64 key column k, and the value columns i64 / f64 / dec of TA.make_table (NULLs at 0.3)"""
    n = len(k)
    cols = {"id": pa.array(np.arange(n, dtype=np.int64)), "k": pa.array(np.asarray(k, np.int64), pa.int64())}
    if n_extra:
        base = TA.make_table(n, 0.3)
        for c in ("g", "i64", "f64", "dec"):
            cols[c] = base.column(c)
    return pa.table(cols)


def check_all(k, got, keep, what):
    """every group: first-appearance order, COUNT_ROWS, SUM / MIN / MAX of id -- `got` begins with ID_SPECS"""
    want_keys, numbers = WM.group_numbers(np.asarray(k, np.int64), keep)
    assert [keys[0] for keys, _ in got] == want_keys.tolist(), (what, len(got), len(want_keys))
    rows = np.flatnonzero(keep)
    n = len(want_keys)
    count, total = np.zeros(n, np.int64), np.zeros(n, np.int64)
    np.add.at(count, numbers[rows], 1)
    np.add.at(total, numbers[rows], rows)                   # (row ids below 2^20: the sums stay far inside int64)
    lo, hi = np.full(n, np.iinfo(np.int64).max), np.full(n, -1, np.int64)
    np.minimum.at(lo, numbers[rows], rows)
    np.maximum.at(hi, numbers[rows], rows)
    assert [vals[:4] for _, vals in got] == [[int(c), int(t), int(a), int(b)] for c, t, a, b in zip(count, total, lo, hi)], what
    return numbers


def check_sample(table, specs, got, numbers, what, seed=1):
    """at most 32 groups picked by `seed`, and the first and the last: every value against the models"""
    n = len(got)
    pick = set(np.random.default_rng(seed).choice(n, min(n, 32), replace=False).tolist()) | ({0, n - 1} if n else set())
    for g in sorted(pick):
        sub = table.filter(pa.array(numbers == g))
        TX.check(sub, specs, got[g][1], np.ones(sub.num_rows, bool), (what, got[g][0]))


def check_int_keyed(table, specs, got, keep, what):
    numbers = check_all(table.column("k").to_numpy(), got, keep, what)
    check_sample(table, specs, got, numbers, what)


# ---- group counts at the edges of the limit ----
def test_group_counts_at_the_limit():
    n = 1025
    specs = ID_SPECS + TA.specs_for(["i64", "f64", "dec"])[1:]
    for n_groups in (257, 300):
        table = int_table(np.arange(n) % n_groups - 7)
        data, _ = TA.own_file(table)
        got, _, d2h = run(data, table.column_names, specs, ["k"], n_groups)
        assert len(got) == n_groups and d2h == 0
        check_int_keyed(table, specs, got, np.ones(n, bool), n_groups)
    # 301 groups under a limit of 300: refused with the limit that was set, with and without read-ahead
    table = int_table(np.arange(n) % 301, n_extra=False)
    data, _ = TA.own_file(table)
    for prefetch in (0, 2):
        r = TA.builder(data, ["id", "k"], prefetch=prefetch).aggregating_reader(ID_SPECS, group_by=["k"], max_groups=300)
        TG.refused(r.aggregate, UNSUPPORTED, "300")
        r.close()
    pred = P.lt("id", V.Int64(300))                        # the 301st group only among rows the filter drops
    got, _, _ = run(data, ["id", "k"], ID_SPECS, ["k"], 300, pred=pred)
    check_all(table.column("k").to_numpy(), got, AM.kept_mask(table, pred), "301st dropped")
    assert len(got) == 300


def test_every_row_a_group_of_its_own():
    n = 5000
    table = int_table((np.arange(n) * 7919) % 100003, n_extra=False)
    data, _ = TA.own_file(table)
    got, (seen, kept), d2h = run(data, ["id", "k"], ID_SPECS, ["k"], 8192)
    assert len(got) == n and (seen, kept, d2h) == (n, n, 0)
    check_all(table.column("k").to_numpy(), got, np.ones(n, bool), "singletons")
    r = TA.builder(data, ["id", "k"]).aggregating_reader(ID_SPECS, group_by=["k"], max_groups=4999)       # one group too many, far past 256
    TG.refused(r.aggregate, UNSUPPORTED, "4999")
    r.close()


# ---- shapes of segments ----
def threshold_keys():
    """groups of exactly WM.THRESHOLD_COUNTS rows each -- the counts at which the fold rule changes what it does --, their rows
    dealt round-robin so that every group's rows are spread over the words"""
    left = {g: c for g, c in enumerate(WM.THRESHOLD_COUNTS)}
    k = []
    while left:
        for g in sorted(left):
            k.append(g * 1000)
            left[g] -= 1
            if not left[g]:
                del left[g]
    return np.array(k)


def shapes():
    n = 4097
    ids = np.arange(n)
    big = (ids * 3000) // n != ((ids + 1) * 3000) // n       # 3000 rows dealt evenly: some 47 in every word of 64
    skew = np.where(big, 10 ** 6, ids + 10 ** 7)             # one group of 3000 rows and 1097 singletons
    return {"interleaved": ids % 1000, "sorted": np.sort(ids % 1000), "skewed": skew, "thresholds": threshold_keys()}


@pytest.mark.parametrize("shape", ("interleaved", "sorted", "skewed", "thresholds"))
def test_segment_shapes_under_every_arm(shape):
    k = shapes()[shape]
    n = len(k)
    table = int_table(k)
    if shape == "thresholds":
        assert sorted(np.unique(k, return_counts=True)[1].tolist()) == sorted(WM.THRESHOLD_COUNTS)
    if shape == "skewed":
        counts = np.unique(k, return_counts=True)[1]
        assert counts.max() == 3000 and (counts == 1).sum() == 1097 and all((k[w * 64:w * 64 + 64] == 10 ** 6).sum() >= 40 for w in range(n // 64))
    data, _ = TA.own_file(table)
    specs = ID_SPECS + [Agg.sum("i64"), Agg.sum("f64"), Agg.sum("dec"), Agg.min("f64"), Agg.max("dec"), Agg.count("i64")]
    for name, pred, sel in TA.arms(n):
        keep = AM.kept_mask(table, pred, sel, BATCH)
        got, (seen, kept), d2h = run(data, table.column_names, specs, ["k"], 4200, pred=pred, selection=sel)
        assert d2h == 0 and kept == int(keep.sum()), (shape, name)
        if not keep.any():
            assert got == []
            continue
        check_int_keyed(table, specs, got, keep, (shape, name))


# ---- radix pass boundaries ----
def test_group_numbers_that_differ_only_above_bit_8():
    n = 4096 + 65
    ids = np.arange(n)
    k = np.where(ids < 512, ids, (ids % 2) * 256 + (ids // 2) % 256)     # groups 0 .. 511 appear in order; then neighbours are 256 apart
    table = int_table(k)
    data, _ = TA.own_file(table)
    specs = ID_SPECS + [Agg.sum("f64")]
    got, _, _ = run(data, table.column_names, specs, ["k"], 512)
    assert [keys[0] for keys, _ in got] == list(range(512))
    check_int_keyed(table, specs, got, np.ones(n, bool), "256 apart")


def raw_records(src, names, specs, group_by, max_groups, max_total=None, **kw):
    raw = TA.builder(src, names, **kw).aggregate(specs, raw=True, group_by=group_by, max_groups=max_groups, max_total_groups=max_total)
    return [(keys, [(v.kind, v.is_null, v.overflow, v.scale_or_unit, tuple(v.w), struct.pack("<d", v.f)) for v in vals]) for keys, vals in raw]


def test_three_passes_give_the_answer_of_two():
    n = 5000
    table = int_table((np.arange(n) * 7919) % 100003)
    data, _ = TA.own_file(table)
    specs = ID_SPECS + [Agg.sum("f64"), Agg.sum("dec")]
    two = raw_records(data, table.column_names, specs, ["k"], 8192)            # 13 bits: two passes
    three = raw_records(data, table.column_names, specs, ["k"], 70000, 70000)  # 17 bits: three (the total may not lie below the limit of one stripe)
    assert len(two) == n and two == three


# ---- keys ----
def test_every_key_kind_on_the_wide_path(tmp_path):
    capi.load()
    n = 1025
    table = TG.kinds_table(n, 0.3)
    path = str(tmp_path / "kinds.orc")
    orc.write_table(table, path, compression="uncompressed", stripe_size=64 << 20)
    specs = [Agg.count_rows(), Agg.count("i64"), Agg.sum("i64"), Agg.min("dec"), Agg.max("f64"), Agg.sum("dec")]
    for key in TG.KEY_KINDS:
        got, _, d2h = run(path, ["id", "i64", "f64", "dec", key], specs, [key], 1000)
        TG.check_groups(table, specs, [key], got, np.ones(n, bool), key)
        assert d2h == 0 and (None,) in [k for k, _ in got]


def strings_table(n=1025):
    ids = np.arange(n)
    s = [None if x % 311 == 5 else "" if x % 311 == 7 else "k%03d" % (x % 311) + "é" * (x % 311 % 3) for x in ids]       # 311 values: NULL and "" among them
    b = [None if x % 5 == 0 else bool(x % 2) for x in ids]
    return pa.table({"id": pa.array(ids.astype(np.int64)), "s": pa.array(s, pa.string()), "b": pa.array(b, pa.bool_()),
                     "i": pa.array((ids % 7).astype(np.int32), pa.int32()), "d": pa.array([D(int(x % 11)).scaleb(-2) for x in ids], pa.decimal128(15, 2)),
                     "f64": TA.make_table(n, 0.3).column("f64")})


def test_string_keys_and_key_tuples_past_256():
    table = strings_table()
    n = table.num_rows
    data, _ = TA.own_file(table)
    specs = [Agg.count_rows(), Agg.sum("id"), Agg.min("id"), Agg.sum("f64")]
    keep = np.ones(n, bool)
    got, _, _ = run(data, table.column_names, specs, ["s"], 1024)
    assert len(got) == 311 and ("",) in [k for k, _ in got] and (None,) in [k for k, _ in got]
    TG.check_groups(table, specs, ["s"], got, keep, "s")
    for group_by in (["s", "b"], ["i", "s", "b", "d"]):
        pred = P.gte("id", V.Int64(40))
        got, _, _ = run(data, table.column_names, specs, group_by, 2048, pred=pred)
        want = GM.group_rows(table, group_by, AM.kept_mask(table, pred))
        assert len(want) > 256
        assert [tuple(GM.key_id(k) for k in keys) for keys, _ in got] == [tuple(GM.key_id(k) for k in keys) for keys, _ in want], group_by
        assert [v[:3] for _, v in got] == [[int(m.sum()), int(np.flatnonzero(m).sum()), int(np.flatnonzero(m)[0])] for _, m in want]


def test_a_65_byte_string_key_on_the_wide_path():
    n = 600
    s = ["x%03d" % (k % 300) + "y" * 60 for k in range(n)]              # 64 bytes each, 300 values
    s[400] = "z" * 65
    table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "s": pa.array(s, pa.string())})
    data, _ = TA.own_file(table)
    specs = [Agg.count_rows(), Agg.sum("id")]
    drop = P.ne("id", V.Int64(400))
    got, _, _ = run(data, ["id", "s"], specs, ["s"], 512, pred=drop)       # the 65 bytes only in a dropped row: accepted
    assert len(got) == 300 and all(len(k[0].encode()) == 64 for k, _ in got)
    assert got == [((s[i],), [1 if i == 100 else 2, i if i == 100 else 2 * i + 300]) for i in range(300)]
    r = TA.builder(data, ["id", "s"]).aggregating_reader(specs, group_by=["s"], max_groups=512)
    TG.refused(r.aggregate, UNSUPPORTED, "'s'", "64")
    r.close()


# ---- every aggregate kind ----
def test_every_aggregate_kind_on_the_wide_path():
    n = 2049
    base = TA.make_table(n, 0.3)
    k = (np.arange(n) * 31) % 600
    cols = {"id": base.column("id"), "k": pa.array(k.astype(np.int64)), "g": base.column("g")}
    for c in ("i64", "f64", "dec", "i32", "f32"):
        cols[c] = base.column(c)
    table = pa.table(cols)
    data, _ = TA.own_file(table)
    specs = ID_SPECS + TA.specs_for(["i64", "f64", "dec"])[1:] + [Agg.sum(col("i32") * col("i32")), Agg.avg("dec"), Agg.avg("i64"), Agg.avg(col("f64") * col("f32")),
                                                                 Agg.sum(col("f32") * 2.0), Agg.sum(col("dec") * col("dec") + 1)]
    for pred in (None, P.lt("g", V.Int64(1))):
        keep = AM.kept_mask(table, pred)
        got, _, d2h = run(data, table.column_names, specs, ["k"], 600, pred=pred)
        assert d2h == 0
        check_int_keyed(table, specs, got, keep, ("kinds", pred is not None))


def test_a_decimal_overflow_stays_in_its_group():
    n = 1025
    k = np.arange(n) % 300
    d = [10 ** 37 if x == 777 else x % 97 for x in range(n)]           # row 777 (group 177): 10^37 * 10^37 leaves 128 bits
    table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "k": pa.array(k.astype(np.int64)), "d": pa.array([D(v) for v in d], pa.decimal128(38, 0))})
    data, _ = TA.own_file(table)
    specs = ID_SPECS + [Agg.sum(col("d") * col("d")), Agg.sum("d")]
    got, _, _ = run(data, table.column_names, specs, ["k"], 300)
    check_all(k, got, np.ones(n, bool), "overflow")
    for (key,), vals in got:
        rows = np.flatnonzero(k == key)
        if key == 177:
            assert vals[4] == AM.OVERFLOW and vals[5] == D(sum(d[r] for r in rows))
        else:
            assert vals[4:] == [D(sum(d[r] * d[r] for r in rows)), D(sum(d[r] for r in rows))], key
    with pytest.raises(OverflowError) as e:
        TA.builder(data, table.column_names).aggregate(specs, group_by=["k"], max_groups=300)
    assert "(177,)" in str(e.value)


# ---- determinism and the fold rule ----
def mixed_doubles(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)      # sixteen orders of magnitude: the order of summation shows


def test_double_sums_bit_for_bit_against_the_model_of_the_fold_rule():
    for name, k in (("thresholds", threshold_keys()), ("skewed", shapes()["skewed"]), ("interleaved", shapes()["interleaved"])):
        n = len(k)
        x = mixed_doubles(n, 21).tolist()
        xn = [None if i % 5 == 3 else v for i, v in enumerate(x)]
        table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "g": pa.array((np.arange(n) % 7 - 3).astype(np.int64)), "k": pa.array(k.astype(np.int64)),
                          "x": pa.array(x, pa.float64()), "xn": pa.array(xn, pa.float64())})
        data, _ = TA.own_file(table)
        specs = ID_SPECS + [Agg.sum("x"), Agg.sum("xn"), Agg.count("xn")]
        for pred in (None, P.lt("g", V.Int64(1))):
            keep = AM.kept_mask(table, pred)
            raw = TA.builder(data, table.column_names, pred=pred).aggregate(specs, raw=True, group_by=["k"], max_groups=4200)
            numbers = check_all(k, [(keys, [A.value_of(v, s) for v, s in zip(vals[:4], specs)]) for keys, vals in raw], keep, name)
            for g, (keys, vals) in enumerate(raw):
                rows = np.flatnonzero(numbers == g)
                want, _ = WM.fold_f64([x[r] for r in rows])
                assert struct.pack("<d", vals[4].f) == struct.pack("<d", want), (name, keys, len(rows), vals[4].f, want)
                want, count = WM.fold_f64([xn[r] for r in rows])
                assert vals[6].w[0] == count
                if count:
                    assert struct.pack("<d", vals[5].f) == struct.pack("<d", want), (name, keys, len(rows))
                else:
                    assert vals[5].is_null


def test_float32_columns_and_expressions_within_the_bound():
    n = 2049
    base = TA.make_table(n, 0.3)
    table = pa.table({"id": base.column("id"), "k": pa.array(((np.arange(n) * 13) % 400).astype(np.int64)), "f32": base.column("f32"), "f64": base.column("f64")})
    data, _ = TA.own_file(table)
    specs = ID_SPECS + [Agg.sum("f32"), Agg.sum_product("f32", "f64"), Agg.sum(col("f32") * col("f64") - 1.5), Agg.avg("f32")]
    got, _, _ = run(data, table.column_names, specs, ["k"], 400)
    check_int_keyed(table, specs, got, np.ones(n, bool), "f32")


CHILD = r'''
import hashlib, io, os, struct, sys
sys.path.insert(0, %r)
import numpy as np, pyarrow as pa
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.arrow_writer import ArrowWriterBuilder
n = 4097
ids = np.arange(n)
k = np.where(ids %% 4 != 1, 10 ** 6, ids)
rng = np.random.default_rng(21)
x = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, n)
table = pa.table({"id": pa.array(ids.astype(np.int64)), "k": pa.array(k.astype(np.int64)), "s": pa.array(["v%%d" %% (v %% 300) for v in ids], pa.string()),
                  "x": pa.array(x.tolist(), pa.float64())})
ctx = capi.Context()
out = io.BytesIO()
w = ArrowWriterBuilder(out, table.schema, ctx=ctx).try_build()
for batch in table.to_batches():
    w.write(batch)
w.close()
w.free()
data = out.getvalue()
specs = [Agg.count_rows(), Agg.sum("x"), Agg.sum("id"), Agg.max("id")]
h = hashlib.sha256()
for group_by in (["k"], ["s", "k"]):
    for _ in range(2):      # (the second call reuses the workspace: what POISON is about)
        b = ArrowReaderBuilder.try_new(data, ctx).with_batch_size(1024).with_prefetch(0).with_projection(table.column_names)
        raw = b.aggregate(specs, raw=True, group_by=group_by, max_groups=4200)
        h.update(repr([(keys, [(v.kind, v.is_null, tuple(v.w), struct.pack("<d", v.f)) for v in vals]) for keys, vals in raw]).encode())
print("GROUPS", len(raw), "DIGEST", h.hexdigest())
''' % (ROOT,)


def digest(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("ORCGPU_")}
    env.update(extra)
    p = subprocess.run([sys.executable, "-c", CHILD], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    return [line for line in p.stdout.decode().splitlines() if line.startswith("GROUPS")][-1]


def test_the_same_records_on_every_run_under_few_hash_bits_and_under_poison():
    # the same call twice in this process: identical raw records, Float sums by their bits
    k = shapes()["skewed"]
    n = len(k)
    table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "k": pa.array(k.astype(np.int64)), "x": pa.array(mixed_doubles(n, 21).tolist(), pa.float64())})
    data, _ = TA.own_file(table)
    specs = ID_SPECS + [Agg.sum("x")]
    runs = [raw_records(data, table.column_names, specs, ["k"], 4200) for _ in range(2)]
    assert runs[0] == runs[1] and len(runs[0]) > 256
    # ... and in child processes (one that faults or times out fails the assert in digest(): no further child is started)
    plain = digest({})
    assert int(plain.split()[1]) > 1025                          # (the last key list: every singleton, and the big group by `s`)
    assert digest({"ORCGPU_GROUP_HASH_BITS": "4"}) == plain       # sixteen hash values for a thousand keys: long probe sequences
    assert digest({"ORCGPU_POISON": "0xA5"}) == plain


# ---- several stripes ----
def test_stripes_that_share_groups_and_add_new_ones():
    n = 3 * 1025 + 7
    ids = np.arange(n)
    stripe = np.searchsorted([n * 1 // 3, n * 2 // 3], ids, side="right")        # (where TA.own_file cuts)
    k = (ids * 17) % 300 + stripe * 150                     # every stripe 300 groups, 150 of them the next stripe's too: 600 in all
    table = int_table(k)
    data, rows = TA.own_file(table, stripes=3)
    assert orc.ORCFile(io.BytesIO(data)).nstripes == 3
    specs = ID_SPECS + [Agg.sum("i64"), Agg.sum("dec"), Agg.min("dec"), Agg.sum("f64")]
    names = table.column_names
    parts, at = [], 0
    for r in rows:
        part_keep = np.zeros(n, bool)
        part_keep[at:at + r] = True
        parts.append(GM.group_rows(table, ["k"], part_keep))
        at += r
    assert all(len(p) > 256 for p in parts)
    order = GM.merge_stripes(parts)
    assert len(order) == 600
    for prefetch in (0, 2):
        got, (seen, kept), d2h = run(data, names, specs, ["k"], 300, max_total=600, prefetch=prefetch)       # exactly the total: accepted
        assert [keys for keys, _ in got] == order and d2h == 0 and (seen, kept) == (n, n)
        check_all(k, got, np.ones(n, bool), "stripes")          # (stripes are runs of rows: the merged order is the table's first-appearance order)
        for g in (0, 299, 300, 449, 599):                       # groups of one stripe and of two
            mask = k == got[g][0][0]
            exact = [(sp, v) for sp, v in zip(specs, got[g][1]) if not isinstance(v, float)]      # (float sums merge in stripe order: other bits)
            assert [v for _, v in exact] == [AM.aggregate_one(table, sp, mask) for sp, _ in exact], g
            TX.check(table, specs, got[g][1], mask, ("stripes", got[g][0]))
        r = TA.builder(data, names, prefetch=prefetch).aggregating_reader(specs, group_by=["k"], max_groups=300, max_total_groups=599)
        TG.refused(r.aggregate, UNSUPPORTED, "599")              # one less: refused, the limit in the message
        r.close()


# ---- the wide path on few groups ----
def test_few_groups_on_the_wide_path_are_the_narrow_paths_groups():
    n = 1025
    table = TG.keyed_table(n)
    names = ["id", "g", "flag", "status", "half", "i64", "f64", "dec"]
    data, _ = TA.own_file(table.select(names))
    specs = TA.specs_for(names)
    for name, pred, sel in TA.arms(n):
        keep = AM.kept_mask(table, pred, sel, BATCH)
        wide, _, _ = run(data, names, specs, ["flag", "status"], 1000, pred=pred, selection=sel)
        narrow, _, _ = TG.run(data, names, specs, ["flag", "status"], pred=pred, selection=sel)
        assert [k for k, _ in wide] == [k for k, _ in narrow], name
        for (_, a), (_, b) in zip(wide, narrow):
            assert [x for x in a if not isinstance(x, float)] == [x for x in b if not isinstance(x, float)], name       # exact values: the same
        TG.check_groups(table, specs, ["flag", "status"], wide, keep, ("few", name))                                    # Float sums: to the tolerance


# ---- stripe level ----
def test_result_aggregate_groups_with_a_limit_agrees_with_the_reader():
    n = 4097
    c = TA.ctx()
    res, table = TA.stripe_result(n, 1000)
    specs = [Agg.count_rows(), Agg.count("v"), Agg.sum("v"), Agg.min("v"), Agg.max("v"), Agg.sum_product("v", "id")]
    pred = P.gte("id", V.Int64(64))
    for p in (None, pred):
        got = c.result_aggregate_groups(res, specs, ["id"], ["id", "v"], p, max_groups=4097)        # every row a group
        v = table.column("v").to_pylist()
        assert got == [((i,), [1, 0, None, None, None, None] if v[i] is None else [1, 1, v[i], v[i], v[i], v[i] * i]) for i in range(64 if p is not None else 0, n)]
        wide = c.result_aggregate_groups(res, specs, ["v"], ["id", "v"], p, max_groups=300)           # ~100 groups and the NULL key
        assert wide == c.result_aggregate_groups(res, specs, ["v"], ["id", "v"], p) == GM.aggregate_groups(table, specs, ["v"], p)
    with pytest.raises(capi.OrcGpuError) as e:
        c.result_aggregate_groups(res, specs, ["id"], ["id", "v"], max_groups=4096)
    assert e.value.code == UNSUPPORTED and "4096" in str(e.value)
    data, _ = TA.own_file(table)
    got, _, _ = run(data, ["id", "v"], specs, ["v"], 300)
    assert got == c.result_aggregate_groups(res, specs, ["v"], ["id", "v"], max_groups=300)
    res.free()
