"""The row filter's expression leaf on the GPU (Predicate.compare: lhs OP rhs; filter_expr_kernel in device/filter_kernels.hip,
the two sides compiled by orcgpu_agg_expr.inc) against the model of tests/filter_model_expr.py: the rows the model keeps of the
reader's own unfiltered read are what the reader must hand out under the filter -- as the row filter, as an aggregate's condition
and as the filter of a top-k.  Files are written with pyarrow.orc, a few thousand rows at most."""
import decimal
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import filter_model_expr as M
import selection_model as SM
from orc_rust_amd import capi
from orc_rust_amd.predicate import AND as PR_AND
from orc_rust_amd.aggregate import Agg, col, lit
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = decimal.Decimal
EXACT = decimal.Context(prec=80)
OPS = ("=", "!=", "<", "<=", ">", ">=")
NAN, INF = float("nan"), float("inf")
BIG = 10 ** 37
DEC = {"p": (12, 2), "q": (20, 7), "w": (38, 0), "v": (38, 0), "z": (38, 20)}
SCHEMA = {"id": "int", "a": "int", "b": "int", "i32": "int", "d1": "int", "d2": "int", "g": "int", "k": "int", "x": "float", "y": "float", "f": "float"}
SCHEMA.update({name: ("dec", s) for name, (_, s) in DEC.items()})
_CTX = None
_TABLES = {}


def ctx():
    global _CTX
    if _CTX is None:
        _CTX = capi.Context()
    return _CTX


def columns(n, null_frac, seed=11):
    """name -> a list of Python values as the model reads them (ints, a Decimal's unscaled int, floats; None: NULL)"""
    rng = np.random.default_rng(seed + n)

    def nulls(values, keep_all=False):
        if keep_all or null_frac == 0.0:
            return list(values)
        return [None if m else v for v, m in zip(values, rng.random(n) < null_frac)]

    def pick(pool):
        return [pool[k] for k in rng.permutation(n) % len(pool)]

    floats = [0.0, -0.0, 1.5, -1.5, NAN, INF, -INF, 0.1, 0.2, 0.30000000000000004, 1e308, 10.0, 1e-320]
    out = {"id": list(range(n)), "g": [int(v) for v in rng.integers(0, 5, n)], "k": [int(v) % 300 for v in rng.permutation(n)]}
    out["a"] = [int(v) for v in rng.integers(-20, 21, n)]
    out["b"] = nulls([int(v) for v in rng.integers(-20, 21, n)])
    out["i32"] = nulls([int(v) for v in rng.integers(-5, 6, n)])
    out["d1"] = nulls([int(v) for v in rng.integers(8000, 8100, n)])
    out["d2"] = nulls([int(v) for v in rng.integers(8000, 8160, n)])
    out["p"] = nulls(pick([150, 199, -1, 0, 10 ** 12 - 1, 1 - 10 ** 12, 5, 100]))
    out["q"] = nulls(pick([15000000, 19900000, 19900001, -100000, 0, 10 ** 20 - 1, 50000, 1000000000]))
    out["w"] = nulls(pick([BIG, -BIG, 0, 17, -17, 10 ** 38 - 1, 1 - 10 ** 38, 3]))
    out["v"] = nulls(pick([BIG, 3, -BIG, 1, 0, -(10 ** 20), 10 ** 19, 2]))
    out["z"] = nulls(pick([5, -5, 0, 17 * 10 ** 20, -17 * 10 ** 20, 10 ** 38 - 1, 1 - 10 ** 38, 3 * 10 ** 20]))
    out["x"] = nulls(pick(floats))
    out["y"] = nulls(pick(floats[::-1] + [2.0]))
    out["f"] = nulls(pick([float(np.float32(v)) for v in (0.1, 1.5, -0.0, NAN, INF, 3.0)]))
    out["s"] = ["%s%d" % ("ab"[i % 2], i % 7) for i in range(n)]
    return out


def table_of(n, null_frac=0.25):
    """(path-free) -> the ORC bytes, the columns as the model reads them, and the reader's own unfiltered read"""
    key = (n, null_frac)
    if key not in _TABLES:
        c = columns(n, null_frac)
        arrays = {}
        for name, vals in c.items():
            if name in DEC:
                p, s = DEC[name]
                arrays[name] = pa.array([None if v is None else D(v).scaleb(-s, EXACT) for v in vals], pa.decimal128(p, s))
            elif name in ("d1", "d2"):
                arrays[name] = pa.array(vals, pa.date32())
            elif name == "i32":
                arrays[name] = pa.array(vals, pa.int32())
            elif name == "f":
                arrays[name] = pa.array(vals, pa.float32())
            elif name in ("x", "y"):
                arrays[name] = pa.array(vals, pa.float64())
            elif name == "s":
                arrays[name] = pa.array(vals, pa.string())
            else:
                arrays[name] = pa.array(vals, pa.int64())
        sink = pa.BufferOutputStream()
        orc.write_table(pa.table(arrays), sink, compression="uncompressed", row_index_stride=1000)
        data = sink.getvalue().to_pybytes()
        rows = [{name: vals[i] for name, vals in c.items()} for i in range(n)]
        plain = tab(read(data)[0])
        assert plain.num_rows == n and plain.column("id").to_pylist() == c["id"]
        _TABLES[key] = (data, rows, plain)
    return _TABLES[key]


def read(src, pred=None, batch_size=1000, prune=False, selection=None):
    b = ArrowReaderBuilder.try_new(src, ctx()).with_batch_size(batch_size)
    if selection is not None:
        b = b.with_row_selection(selection)
    if pred is not None:
        b = b.with_row_filter(pred, prune=prune)
    r = b.build()
    try:
        return list(r), r.filter_rows(), r.filter_overflow_rows(), r.row_groups()
    finally:
        r.close()


def same(t1, t2):
    """two tables, equal column by column: names, types and values -- the float columns by their values' spelling, so that a NaN
    equals a NaN and -0.0 is not 0.0.  (A field's nullability is not compared: kept rows without a null say "not null".)"""
    if t1.column_names != t2.column_names or [f.type for f in t1.schema] != [f.type for f in t2.schema] or t1.num_rows != t2.num_rows:
        return False
    for c in t1.column_names:
        a, b = t1.column(c).to_pylist(), t2.column(c).to_pylist()
        if c in ("x", "y", "f"):
            a, b = [repr(v) for v in a], [repr(v) for v in b]
        if a != b:
            return False
    return True


def tab(batches, plain=None):
    """the batches as one table.  (A batch whose rows hold no null says "not null" for the column: the fields are made nullable
    first, so that batches of one read go together.)"""
    if not batches:
        return plain.slice(0, 0)
    schema = pa.schema([pa.field(f.name, f.type) for f in batches[0].schema])
    return pa.concat_tables([pa.Table.from_batches([b]).cast(schema) for b in batches])


def check(n, lhs, op, rhs, null_frac=0.25, batch_size=1000, selection=None, want_overflow=0, under_not=False):
    """the leaf as the row filter, against the model on the rows the selection leaves; returns the kept ids"""
    data, rows, plain = table_of(n, null_frac)
    seen = list(range(n))
    if selection is not None:  # (the rows the reference's stepping of a selection hands out: tests/selection_model.py)
        seen = [i for start, length in SM.file_batches(selection, [n], batch_size)[0] for i in range(start, start + length)]
    truth = [M.evaluate(lhs, op, rhs, rows[i], SCHEMA) for i in seen]
    want = [i for i, (t, _) in zip(seen, truth) if (M.not3(t) if under_not else t) is True]
    overflow = sum(o for _, o in truth)
    leaf = P.compare(lhs, op, rhs)
    batches, (n_seen, n_kept), n_over, _ = read(data, P.not_(leaf) if under_not else leaf, batch_size=batch_size, selection=selection)
    got = tab(batches, plain)
    assert (n_seen, n_kept) == (len(seen), len(want)), (n, lhs, op, rhs)
    assert got.column("id").to_pylist() == want, (n, lhs, op, rhs)
    assert same(got, plain.take(pa.array(want, pa.int64()))), (n, lhs, op, rhs)
    assert all(b.num_rows == batch_size for b in batches[:-1])
    assert n_over == overflow == want_overflow or want_overflow is None and n_over == overflow, (n_over, overflow, want_overflow)
    return want


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4 * 128 - 1, 4 * 128 + 1, 1025))
def test_row_counts_where_trips_blocks_and_batches_end_mid_word(n):
    # (a batch size of 128: two trips a batch, so that batches and input words end together and apart)
    for null_frac in (0.0, 0.25):
        check(n, col("a"), "<", col("b"), null_frac=null_frac, batch_size=128)
        check(n, col("p") * (1 - col("q")), ">", lit(D("-10.5")), null_frac=null_frac, batch_size=128)
    check(n, col("x"), "<=", col("y"), batch_size=128)


def test_a_row_selection_on_top():
    n = 3001
    # (no select longer than a batch: the reference's stepping runs such a one on to the stripe's end)
    selection = [(10, True), (100, False), (7, True), (1, False), (900, True), (256, False), (300, True), (200, False), (1227, True)]
    assert check(n, col("a") + col("i32"), ">=", col("b"), selection=selection, batch_size=256)
    assert check(n, col("w"), ">", col("z"), selection=selection, batch_size=256)
    check(n, col("w") * col("v"), ">", lit(0), selection=selection, batch_size=256, want_overflow=None)


@pytest.mark.parametrize("op", OPS)
def test_all_six_operators_in_the_three_classes_with_nulls_on_either_side(op):
    n = 2049
    kept = check(n, col("b"), op, col("i32"))  # nulls in both
    assert 0 < len(kept) < n
    check(n, col("a"), op, col("b"))           # nulls on the right only
    check(n, col("b") * 2 - 1, op, col("a") + col("i32"))
    kept = check(n, col("p"), op, col("q"))    # Decimal(12, 2) against Decimal(20, 7)
    assert 0 < len(kept) < n
    check(n, col("p") + col("a"), op, col("q") * 2)  # an integer column beside Decimals
    kept = check(n, col("x"), op, col("y"))    # NaN, +-0.0, +-inf on both sides
    assert 0 < len(kept) < n
    check(n, col("f"), op, col("x"))           # a Float column widened
    check(n, col("x") * col("y"), op, col("f") + 0.5)
    # Decimal(38, 0) near 10^37 against Decimal(38, 20): the final rescale leaves 128 bits, the order stays exact, nothing is counted
    kept = check(n, col("w"), op, col("z"))
    assert 0 < len(kept) < n
    check(n, col("z"), op, col("v"))


def test_dates():
    n = 2049
    assert check(n, col("d1"), "<", col("d2"))
    assert check(n, col("d2") - col("d1"), ">", lit(30))
    assert check(n, col("d1") + col("i32"), "=", col("d2"), want_overflow=0) is not None


def test_an_inner_overflow_is_unknown_and_counted():
    n = 2049
    _, rows, _ = table_of(n)
    lhs = col("w") * col("v")
    want_over = sum(M.evaluate(lhs, ">", lit(0), r, SCHEMA)[1] for r in rows)
    assert want_over > 50
    kept = check(n, lhs, ">", lit(0), want_overflow=want_over)
    dropped = check(n, lhs, ">", lit(0), want_overflow=want_over, under_not=True)
    assert kept and dropped and len(kept) + len(dropped) < n - want_over + 1  # the overflowing rows are in neither
    # the scale-up of an addition is an operation like any other
    check(n, col("w") + col("z"), "<", col("p"), want_overflow=None)
    check(n, col("p"), "!=", col("v") * col("w") * col("w"), want_overflow=None)


def kleene_and(xs):
    return False if any(x is False for x in xs) else None if any(x is None for x in xs) else True


def kleene_or(xs):
    return True if any(x is True for x in xs) else None if any(x is None for x in xs) else False


def test_beside_a_like_and_an_in_leaf_under_and_or_not():
    n = 3001
    data, rows, plain = table_of(n)
    e1, e2 = (col("a"), "<", col("b")), (col("w") * col("v"), ">", col("p"))
    pred = P.or_([P.and_([P.compare(*e1), P.like("s", "a%")]), P.not_(P.or_([P.in_list("g", [V.Int64(1), V.Int64(2)]), P.compare(*e2)])),
                  P.and_([P.compare(col("x"), "!=", col("y")), P.in_list("i32", [V.Int32(0), V.Int32(3), V.Int32(None)])])])
    want, overflow = [], 0
    for i, r in enumerate(rows):
        t1, _ = M.evaluate(*e1, r, SCHEMA)
        t2, o2 = M.evaluate(*e2, r, SCHEMA)
        t3, _ = M.evaluate(col("x"), "!=", col("y"), r, SCHEMA)
        overflow += o2
        in32 = None if r["i32"] is None or r["i32"] not in (0, 3) else True
        t = kleene_or([kleene_and([t1, r["s"].startswith("a")]), M.not3(kleene_or([r["g"] in (1, 2), t2])), kleene_and([t3, in32])])
        if t is True:
            want.append(i)
    batches, rows_seen, n_over, _ = read(data, pred, batch_size=512)
    assert tab(batches, plain).column("id").to_pylist() == want and rows_seen == (n, len(want)) and 0 < len(want) < n
    assert n_over == overflow > 0


def test_simple_forms_and_pruning():
    n = 4097
    data, rows, plain = table_of(n)
    for prune in (False, True):
        got = read(data, P.compare(col("id"), "<", lit(5) * 300), prune=prune)
        ref = read(data, P.lt("id", V.Int64(1500)), prune=prune)
        assert same(tab(got[0], plain), tab(ref[0], plain)) and got[1:] == ref[1:]
        got = read(data, P.compare(lit(1500), ">", col("id")), prune=prune)  # mirrored
        assert same(tab(got[0], plain), tab(ref[0], plain)) and got[1:] == ref[1:]
    assert read(data, P.lt("id", V.Int64(1500)), prune=True)[3][0] <= read(data, P.lt("id", V.Int64(1500)), prune=False)[3][0]
    # an expression leaf is a "might match": prune=True keeps what prune=False keeps
    for pred in (P.compare(col("id") + col("a"), "<", lit(1500)), P.and_([P.compare(col("d1"), "<", col("d2")), P.gte("id", V.Int64(3000))]),
                 P.not_(P.compare(col("id") * 2, ">=", col("k")))):
        a, b = read(data, pred, prune=True), read(data, pred, prune=False)
        assert same(tab(a[0], plain), tab(b[0], plain)) and a[1][1] == b[1][1] > 0 and a[2] == b[2] == 0 and b[1][0] == n
        # (the literal leaf beside it may drop row groups, so fewer rows are SEEN; an expression leaf alone keeps every group)
        assert a[1][0] == n or pred.op == PR_AND and a[1][0] < n
    # two literal sides
    assert read(data, P.compare(lit(2) * 3, "=", lit(6)))[1] == (n, n) and read(data, P.compare(lit(D("1.5")), "<", lit(1)))[1] == (n, 0)


def builder(data, pred=None):
    b = ArrowReaderBuilder.try_new(data, ctx()).with_batch_size(1000)
    return b if pred is None else b.with_row_filter(pred, prune=False)


def test_as_an_aggregates_condition_plain_and_grouped():
    n = 3001
    data, rows, _ = table_of(n)
    conds = [(col("a"), "<", col("b")), (col("w") * col("v"), ">", col("p")), (col("x") * 2, ">=", col("y"))]
    specs = []
    for c in conds:
        specs += [Agg.count_rows().where(P.compare(*c)), Agg.sum("a").where(P.not_(P.compare(*c)))]
    specs.append(Agg.count_rows())

    def model(subset):
        out = []
        for c in conds:
            truth = [M.evaluate(*c, rows[i], SCHEMA)[0] for i in subset]
            out += [sum(t is True for t in truth), sum(rows[i]["a"] for i, t in zip(subset, truth) if t is False) if any(t is False for t in truth) else None]
        return out + [len(subset)]

    for pred, subset in ((None, list(range(n))), (P.compare(col("d1"), "<", col("d2")), [i for i in range(n) if M.evaluate(col("d1"), "<", col("d2"), rows[i], SCHEMA)[0] is True])):
        assert builder(data, pred).aggregate(specs) == model(subset)
        for key, max_groups, n_keys in (("g", None, 5), ("k", 400, 300)):  # the default path, and the sorted one past 256 groups
            groups = builder(data, pred).aggregate(specs, group_by=[key], max_groups=max_groups)
            got = {tuple(k)[0]: list(v) for k, v in groups}
            want = {}
            for i in subset:
                want.setdefault(rows[i][key], []).append(i)
            assert len(got) == len(want) <= n_keys and got == {k: model(v) for k, v in want.items()}, (key, max_groups)


def test_as_the_filter_of_a_top_k():
    n = 3001
    data, rows, _ = table_of(n)
    for c in ((col("a") * col("i32"), ">", col("b")), (col("w") * col("v"), ">", col("p")), (col("x"), "<", col("y"))):
        keep = [i for i in range(n) if M.evaluate(*c, rows[i], SCHEMA)[0] is True]
        want = sorted(keep, key=lambda i: (-rows[i]["a"], i))[:25]
        got = builder(data, P.compare(*c)).top_k([("a", "desc"), "id"], 25)
        assert got.column("id").to_pylist() == want and len(want) == 25


CHILD = r'''
import sys
sys.path[:0] = [%r, %r]
import torch
import test_gpu_row_filter_expr as T
out = []
for _ in range(2):      # (the second pass reuses the workspaces: what POISON is about)
    for n in (65, 2049):
        for c in ((T.col("a"), "<", T.col("b")), (T.col("w") * T.col("v"), ">", T.col("p")), (T.col("x"), "!=", T.col("y"))):
            out.append(T.check(n, *c, want_overflow=None, batch_size=256))
print("ANSWER", repr(out))
'''


def test_poison_does_not_show_through_the_planes():
    lines = []
    for extra in ({}, {"ORCGPU_POISON": "0xA5"}):
        env = {k: v for k, v in os.environ.items() if not k.startswith("ORCGPU_")}
        env.update(extra)
        p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-3000:]      # (a child that faults fails here: no further child is started)
        lines.append([ln for ln in p.stdout.decode().splitlines() if ln.startswith("ANSWER")][-1])
    assert lines[0] == lines[1] and len(lines[0]) > 5_000


def test_refusals_arrive_at_the_first_batch():
    data, _, _ = table_of(65)
    for pred, code, name in ((P.compare(col("x"), "<", col("a")), 6, "'x'"), (P.compare(col("s"), "<", col("a")), 7, "'s'"), (P.compare(col("z") * col("z"), "<", col("a")), 7, "'z'")):
        r = builder(data, pred).build()
        with pytest.raises(capi.OrcGpuError) as e:
            list(r)
        assert e.value.code == code and name in str(e.value) and "row filter" in str(e.value)
        r.close()
