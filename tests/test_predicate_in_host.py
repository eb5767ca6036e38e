"""Row-group pruning under an IN leaf (orcgpu_predicate_row_groups, host only) on the ROW_INDEX and Bloom filter streams of files
written with pyarrow: the groups kept for x IN (v1 .. vk) are exactly the union of the groups kept for each x = v, no group that
holds a matching row is dropped, under a NOT every group is kept, a literal of the wrong type fails as EQ does -- and 65536
literals do not cost 65536 tests per group."""
import decimal
import time

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest

from orcfile import BLOOM_FILTER_UTF8, ROW_INDEX, OrcFile
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
from test_predicate_host import evaluate

N, STRIDE = 10000, 1000
D = decimal.Decimal
_FILES = {}


def table():
    rng = np.random.default_rng(41)
    i = np.sort(rng.integers(0, 10 ** 6, N)) * 2                      # sorted: every group has its own range
    s = ["k%07d" % x for x in np.sort(rng.integers(0, 10 ** 6, N)) * 2]
    d = np.sort(rng.integers(-10 ** 5, 10 ** 5, N)) * 0.5
    dec = [D(int(x) * 2).scaleb(-2) for x in np.sort(rng.integers(-10 ** 6, 10 ** 6, N))]
    r = rng.integers(0, 500, N) * 2                                    # unsorted: every group spans everything, the Bloom filter decides
    return pa.table({"i": pa.array(i, pa.int64()), "s": pa.array(s), "d": pa.array(d, pa.float64()), "dec": pa.array(dec, pa.decimal128(10, 2)),
                     "r": pa.array(r, pa.int64())})


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """bloom -> ({column: (ROW_INDEX bytes, Bloom filter bytes or None)}, the table)"""
    if not _FILES:
        d = tmp_path_factory.mktemp("predicate_in")
        t = table()
        for bloom in (False, True):
            path = str(d / ("bloom%d.orc" % bloom))
            kw = {"bloom_filter_columns": list(range(1, t.num_columns + 1))} if bloom else {}  # (the file's column ids: 0 is the root)
            orc.write_table(t, path, compression="uncompressed", stripe_size=64 << 20, row_index_stride=STRIDE, **kw)
            of = OrcFile(path)
            assert len(of.stripes) == 1
            streams = of.stripes[0].streams
            cols = {}
            for k, name in enumerate(t.schema.names):
                bl = streams.get((k + 1, BLOOM_FILTER_UTF8))
                cols[name] = (bytes(streams[(k + 1, ROW_INDEX)]), bytes(bl) if bl is not None else None)
            assert bloom == all(v[1] for v in cols.values())
            _FILES[bloom] = (cols, t)
    return _FILES


def lit(name, v):
    return {"i": V.Int64, "r": V.Int64, "s": V.Utf8, "d": V.Float64, "dec": V.Decimal128}[name](v)


def groups_with(t, name, values):
    col = t.column(name).to_pylist()
    want = set(values)
    return [any(v in want for v in col[g:g + STRIDE]) for g in range(0, N, STRIDE)]


def lists(t, name):
    col = t.column(name).to_pylist()
    rng = np.random.default_rng(7)
    odd = {"i": 1, "r": 1, "d": 0.25, "dec": D("0.01")}
    miss = (lambda v: v + odd[name]) if name != "s" else (lambda v: v + "x")
    out = [[], [col[1500]], [col[1500], col[1501], miss(col[7300])], [miss(col[10]), miss(col[9990])]]
    for size in (3, 16, 200):
        picks = [col[int(k)] for k in rng.integers(0, N, size)]
        out.append([v if k % 2 else miss(v) for k, v in enumerate(picks)])
    return out


@pytest.mark.parametrize("bloom", (False, True))
def test_in_keeps_the_union_of_what_its_eq_leaves_keep(files, bloom):
    cols, t = files[bloom]
    dropped = 0
    for name in t.schema.names:
        for values in lists(t, name):
            got = evaluate(P.in_list(name, [lit(name, v) for v in values]), cols, N, STRIDE)
            union = [False] * (N // STRIDE)
            for v in values:
                one = evaluate(P.eq(name, lit(name, v)), cols, N, STRIDE)
                union = [a or b for a, b in zip(union, one)]
            assert got == union, (name, values[:4], got, union)
            assert all(g or not h for g, h in zip(got, groups_with(t, name, values))), (name, values[:4])  # sound
            dropped += got.count(False)
            assert evaluate(P.not_in(name, [lit(name, v) for v in values]), cols, N, STRIDE) == [True] * (N // STRIDE)
    assert dropped > 100
    # the Bloom filter is what drops groups of the unsorted column
    misses = evaluate(P.in_list("r", [V.Int64(1), V.Int64(3), V.Int64(999)]), cols, N, STRIDE)
    assert misses == ([False] * 10 if bloom else [True] * 10)
    # inside a tree the leaf combines like any other
    both = P.and_([P.in_list("i", [lit("i", t.column("i")[1500].as_py())]), P.in_list("s", [lit("s", t.column("s")[1500].as_py())])])
    assert evaluate(both, cols, N, STRIDE).count(True) >= 1 and evaluate(P.not_(both), cols, N, STRIDE) == [True] * 10


def test_what_fails_fails_as_eq_does(files):
    cols, t = files[True]
    for name, bad in (("i", V.Utf8("a")), ("s", V.Int64(1)), ("d", V.Int64(1)), ("i", V.Int64(None)), ("dec", V.Int64(1))):
        eq = evaluate(P.eq(name, bad), cols, N, STRIDE)
        assert not isinstance(eq, list)
        good = lit(name, t.column(name)[5].as_py())
        assert evaluate(P.in_list(name, [good, bad]), cols, N, STRIDE) == eq, name
        assert evaluate(P.in_list(name, [bad]), cols, N, STRIDE) == eq, name
    assert evaluate(P.in_list("nope", [V.Int64(1)]), cols, N, STRIDE) == evaluate(P.eq("nope", V.Int64(1)), cols, N, STRIDE)
    # the empty list can hold no row, whatever the column
    assert evaluate(P.in_list("i", []), cols, N, STRIDE) == [False] * 10


def test_65536_literals_are_searched_not_looped(files):
    cols, t = files[True]
    col = t.column("i").to_pylist()
    inside = [col[2500], col[2501] + 1, col[8800]]
    top = max(col)
    values = inside + [top + 1 + 2 * k for k in range(65536 - len(inside))]  # all the others lie above every group
    pred = P.in_list("i", [V.Int64(v) for v in values])
    t0 = time.perf_counter()
    got = evaluate(pred, cols, N, STRIDE)
    took = time.perf_counter() - t0
    union = [False] * 10
    for v in inside:
        union = [a or b for a, b in zip(union, evaluate(P.eq("i", V.Int64(v)), cols, N, STRIDE))]
    assert got == union and got.count(True) in (2, 3)
    for v in values[3::1500]:
        assert evaluate(P.eq("i", V.Int64(v)), cols, N, STRIDE) == [False] * 10
    # flattening 65536 nodes in Python is most of it; 65536 x 10 groups x a Bloom filter's probes would be far more
    assert took < 5.0, took
    # the unsorted column: every literal lies inside every group, so every one may be put to the filter -- once per group at most
    rvals = [V.Int64(2 * k + 1) for k in range(65536)]
    t0 = time.perf_counter()
    assert evaluate(P.in_list("r", rvals), cols, N, STRIDE).count(True) <= 10
    assert time.perf_counter() - t0 < 10.0
