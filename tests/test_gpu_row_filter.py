"""The row filter on the GPU (orcgpu_reader_set_row_filter / orcgpu_result_filter: device/filter_kernels.hip) against the model
of tests/filter_model.py: files written here with pyarrow.orc, read back with pyarrow.orc, filtered per stripe by the model and
rebatched -- the reader must hand out exactly those batches."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest

import filter_model as FM
import selection_model as M
from orc_rust_amd import capi
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 1000, 1001, 4097)
BATCH_SIZES = (64, 1000)
COMPRESSIONS = ("uncompressed", "zlib")
_CTX = None
_FILES = {}


def ctx():
    global _CTX
    if _CTX is None:
        _CTX = capi.Context()
    return _CTX


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    capi.load()  # (sets TZDIR where the system has no tz database: pyarrow's ORC writer needs one for the Timestamp column)
    return tmp_path_factory.mktemp("row_filter")


def orc_file(tmpdir, n, compression):
    """(path, the file's rows as pyarrow reads them, rows per stripe)"""
    key = (n, compression)
    if key not in _FILES:
        path = str(tmpdir / ("t%d_%s.orc" % (n, compression)))
        orc.write_table(FM.make_table(n), path, compression=compression, stripe_size=1024, row_index_stride=1000,
                        batch_size=1500 if compression == "uncompressed" else 300)
        f = orc.ORCFile(path)
        rows = [f.read_stripe(i).num_rows for i in range(f.nstripes)]
        # (the zlib writer counts compressed blocks toward the stripe size and cuts this table in two whatever the batch size)
        assert n < 4097 or f.nstripes >= (3 if compression == "uncompressed" else 2), rows
        _FILES[key] = (path, f.read(), rows)
    return _FILES[key]


def read(path, pred=None, batch_size=1000, prune=False, prefetch=0, pruning=True, selection=None, names=None):
    b = ArrowReaderBuilder.try_new(path, ctx()).with_batch_size(batch_size).with_prefetch(prefetch).with_row_group_pruning(pruning)
    if names is not None:
        b = b.with_projection(names)
    if selection is not None:
        b = b.with_row_selection(selection)
    if pred is not None:
        b = b.with_row_filter(pred, prune=prune)
    r = b.build()
    try:
        batches = list(r)
        return batches, r.filter_rows(), r.row_groups()
    finally:
        r.close()


def assert_same_batch(got, want, what):
    """got: a RecordBatch of the reader, want: a Table slice of what pyarrow read.  Floats are compared by their bits on the
    valid rows (NaN is NaN, -0.0 is not 0.0), everything else with equals."""
    assert got.num_rows == want.num_rows, (what, got.num_rows, want.num_rows)
    assert got.schema.names == want.schema.names, what
    got.validate(full=True)
    for name in want.schema.names:
        g, w = got.column(name), want.column(name).combine_chunks()
        assert g.null_count == w.null_count, (what, name, g.null_count, w.null_count)
        if w.null_count == 0:
            assert g.buffers()[0] is None, (what, name, "a column without nulls exports no validity buffer")
        if pa.types.is_floating(w.type):
            assert g.type == w.type, (what, name)
            assert g.is_valid().equals(w.is_valid()), (what, name)
            it = np.int32 if w.type == pa.float32() else np.int64
            gv, wv = (x.fill_null(0).to_numpy(zero_copy_only=False).view(it) for x in (g, w))
            ok = w.is_valid().to_numpy(zero_copy_only=False)
            assert np.array_equal(gv[ok], wv[ok]), (what, name)
        else:
            assert g.cast(w.type).equals(w), (what, name)


def check(path, table, rows, pred, batch_size, selection=None, **kw):
    sel_batches = M.file_batches(selection, rows, batch_size) if selection is not None else None
    want = FM.expected_batches(table, pred, rows, batch_size, sel_batches)
    got, (seen, kept), groups = read(path, pred, batch_size=batch_size, selection=selection, **kw)
    what = (os.path.basename(path), batch_size, kw)
    assert [b.num_rows for b in got] == [w.num_rows for w in want], what
    for k, (g, w) in enumerate(zip(got, want)):
        assert_same_batch(g, w, what + (k,))
    assert kept == sum(w.num_rows for w in want), what
    return got, (seen, kept), groups


def any_of(ids):
    return P.or_([P.eq("id", V.Int64(int(i))) for i in ids])


def core_predicates(n, rows):
    edges = []
    base = 0
    for r in rows:
        edges += [base, base + r - 1]
        base += r
    deep = P.or_([P.and_([P.gte("i32", V.Int32(0)), P.not_(P.or_([P.is_null("s"), P.lt("s", V.Utf8(FM.LITERAL_STRING))]))]),
                  P.and_([P.is_null("i64"), P.not_(P.eq("b", V.Boolean(True)))]), P.lt("f64", V.Float64(-1.0))])
    return {
        "keep-all": P.and_([]),
        "keep-all-by-value": P.gte("id", V.Int64(0)),
        "keep-none": P.or_([]),
        "keep-none-by-value": P.lt("id", V.Int64(0)),
        "row 0": any_of([0]),
        "last row": any_of([n - 1]),
        "rows 63 64 65": any_of([63, 64, 65]),
        "stripe edges": any_of(edges),
        "every 64th": any_of(range(0, n, 64)),
        "all but one": P.ne("id", V.Int64(n // 2)),
        "three deep": deep,
        "not three deep": P.not_(deep),
        "null literal": P.not_(P.eq("i32", V.Int32(None))),
        "long strings": P.gt("s", V.Utf8("mango" + "y" * 10)),
        "all null column": P.or_([P.is_null("allnull"), P.eq("allnull", V.Int32(1))]),
    }


@pytest.mark.parametrize("compression", COMPRESSIONS)
@pytest.mark.parametrize("batch_size", BATCH_SIZES)
@pytest.mark.parametrize("n", SIZES)
def test_row_picks_and_nested_predicates(tmpdir, n, batch_size, compression):
    path, table, rows = orc_file(tmpdir, n, compression)
    for name, pred in core_predicates(n, rows).items():
        got, (seen, kept), _ = check(path, table, rows, pred, batch_size)
        assert seen == n, name
        if name.startswith("keep-all"):
            unfiltered = read(path, None, batch_size=batch_size)[0]
            assert kept == n and len(got) == len(unfiltered)
            for k, (g, u) in enumerate(zip(got, unfiltered)):  # the same rows as the unfiltered reader, batch by batch
                assert_same_batch(g, pa.Table.from_batches([u]), (name, k))
        if name.startswith("keep-none"):
            assert got == [] and (seen, kept) == (n, 0)


@pytest.mark.parametrize("n,batch_size,compression", [(1001, 64, "uncompressed"), (4097, 1000, "zlib")])
def test_every_op_on_every_type(tmpdir, n, batch_size, compression):
    path, table, rows = orc_file(tmpdir, n, compression)
    rng = np.random.default_rng(n)
    for c in FM.ALL_COLUMNS:
        for pred in (P.is_null(c), P.is_not_null(c)):
            check(path, table, rows, pred, batch_size)
    for c in FM.COMPARABLE:
        pool = [v for v in table.column(c).to_pylist() if v is not None]
        literals = [None] + ([pool[int(rng.integers(0, len(pool)))]] if pool else [1])
        if c in ("f32", "f64"):
            literals += [float("nan"), 0.0, -0.0, float("inf")]
        if c == "s":
            literals += ["", FM.LITERAL_STRING, "mango" + "y" * 330, "é"]
        if c == "bin":
            literals += [b"", b"\x80", b"\x7f"]
        for lit in literals:
            for op in range(6):
                check(path, table, rows, P.comparison(c, op, FM.literal_for(table, c, lit)), batch_size)
    # integer columns take every integer literal kind, floats both float kinds, Date both of its kinds
    for mk in (V.Int8, V.Int16, V.Int32, V.Int64):
        check(path, table, rows, P.lte("i64", mk(3)), batch_size)
        check(path, table, rows, P.gt("i8", mk(-7)), batch_size)
    for mk in (V.Float32, V.Float64):
        check(path, table, rows, P.lt("f32", mk(0.1)), batch_size)
        check(path, table, rows, P.gte("f64", mk(0.1)), batch_size)
    for mk in (V.Int32, V.Int64):
        check(path, table, rows, P.lt("d", mk(17)), batch_size)


def test_reader_options_do_not_change_the_batches(tmpdir):
    path, table, rows = orc_file(tmpdir, 4097, "uncompressed")
    preds = [P.and_([P.gte("id", V.Int64(1200)), P.lt("id", V.Int64(1300)), P.is_not_null("s")]),
             P.or_([P.lt("id", V.Int64(10)), P.gt("id", V.Int64(4000))]), P.eq("i32", V.Int32(2)), P.lt("s", V.Utf8("mango"))]
    for pred in preds:
        for prune in (False, True):
            for prefetch in (0, 2):
                for pruning in (True, False):
                    check(path, table, rows, pred, 64, prune=prune, prefetch=prefetch, pruning=pruning)
    _, _, (read_f, total_f) = check(path, table, rows, preds[0], 1000, prune=False)
    _, (seen, kept), (read_t, total_t) = check(path, table, rows, preds[0], 1000, prune=True)
    assert total_f == total_t == read_f and read_t < read_f, (read_t, total_t, read_f, total_f)
    assert kept > 0 and seen < 4097


@pytest.mark.parametrize("compression", COMPRESSIONS)
def test_filter_over_a_row_selection(tmpdir, compression):
    path, table, rows = orc_file(tmpdir, 4097, compression)
    selections = [[(5, True), (60, False), (1000, True), (700, False), (2000, True), (300, False)],
                  [(1, False), (4095, True), (1, False)], [(4097, False)], [(100, True), (1, False), (63, True), (65, False)]]
    preds = [P.and_([]), P.eq("b", V.Boolean(True)), P.or_([P.is_null("f32"), P.gt("s", V.Utf8("m"))]), P.lt("id", V.Int64(0))]
    for sel in selections:
        for pred in preds:
            for batch_size in BATCH_SIZES:
                for prefetch, pruning in ((0, True), (2, False)):
                    check(path, table, rows, pred, batch_size, selection=sel, prefetch=prefetch, pruning=pruning)


def test_an_unfiltered_reader_gives_the_batches_it_always_gave(tmpdir):
    for n, compression in ((4097, "uncompressed"), (4097, "zlib"), (65, "zlib")):
        path, table, rows = orc_file(tmpdir, n, compression)
        for batch_size in BATCH_SIZES:
            got, (seen, kept), _ = read(path, None, batch_size=batch_size)
            want = FM.rebatch(table, rows, batch_size)
            assert (seen, kept) == (0, 0) and len(got) == len(want)
            for k, (g, w) in enumerate(zip(got, want)):
                assert_same_batch(g, w, (n, compression, batch_size, k))


def test_refusals_are_loud_and_name_the_column(tmpdir):
    path, table, rows = orc_file(tmpdir, 1001, "uncompressed")
    deep = P.eq("id", V.Int64(1))
    for _ in range(70):
        deep = P.not_(deep)
    cases = [(P.lt("ts", V.Int64(0)), 7, "ts"), (P.eq("dec", V.Int64(0)), 7, "dec"), (P.eq("nope", V.Int32(1)), 101, "nope"),
             (P.is_null("nope"), 101, "nope"), (P.eq("s", V.Int32(1)), 6, "s"), (P.and_([P.is_null("id"), P.eq("i32", V.Utf8("1"))]), 6, "i32"),
             (deep, 101, "deep")]
    for pred, code, word in cases:
        for prefetch in (0, 2):
            r = ArrowReaderBuilder.try_new(path, ctx()).with_prefetch(prefetch).with_row_filter(pred, prune=False).build()
            with pytest.raises(capi.OrcGpuError) as e:
                next(r)
            assert e.value.code == code and word in str(e.value), (code, word, str(e.value))
            with pytest.raises(StopIteration):  # the iterator has ended
                next(r)
            r.close()
    # a leaf on a column outside the projection is a column that is not there
    r = ArrowReaderBuilder.try_new(path, ctx()).with_projection(["id", "s"]).with_row_filter(P.eq("i32", V.Int32(1)), prune=False).build()
    with pytest.raises(capi.OrcGpuError) as e:
        next(r)
    assert e.value.code == 101 and "i32" in str(e.value)
    r.close()
    # a nested column in the projection
    nested = str(tmpdir / "nested.orc")
    orc.write_table(pa.table({"id": pa.array([1, 2, 3], pa.int64()), "l": pa.array([[1], [], None], pa.list_(pa.int32()))}), nested)
    r = ArrowReaderBuilder.try_new(nested, ctx()).with_row_filter(P.eq("id", V.Int64(1)), prune=False).build()
    with pytest.raises(capi.OrcGpuError) as e:
        next(r)
    assert e.value.code == 7 and "'l'" in str(e.value)
    r.close()
    got, _, _ = read(nested, P.eq("id", V.Int64(2)), names=["id"])  # ... and without it the same file filters
    assert [b.column("id").to_pylist() for b in got] == [[2]]


def test_result_filter_through_the_c_abi():
    """orcgpu_result_filter straight after orcgpu_stripe_decode: views copied with orcgpu_result_copy_batch, then
    orcgpu_result_fetch and orcgpu_result_export_batch on the filtered result; a selected result filters too."""
    from orc_rust_amd import gen
    rng = np.random.default_rng(3)
    n, batch = 4097, 1000
    present = (rng.random(n) > 0.3).astype(np.uint8)
    vals = rng.integers(-50, 50, int(present.sum())).astype(np.int64)
    ids = np.arange(n, dtype=np.int64)
    cols = [{"column_id": 1, "orc_type": 4, "encoding": 2}, {"column_id": 2, "orc_type": 4, "encoding": 2}]
    streams = [(1, 1, gen.rle2(ids, signed=True)), (2, 0, gen.boolean(present)), (2, 1, gen.rle2(vals, signed=True))]
    full = np.zeros(n, dtype=np.int64)
    full[present == 1] = vals
    c = ctx()
    pred = P.and_([P.gt("v", V.Int64(10)), P.gte("id", V.Int64(64))])
    for selection in (None, [(100, True), (2000, False), (1000, True), (997, False)]):
        staged = c.stage(n, streams, cols, batch_size=batch)
        res = c.decode([staged])[0]
        staged.free()
        in_rows = ids
        if selection is not None:
            res.select(selection)
            in_rows = np.concatenate([np.arange(s, s + k) for s, k in M.stripe_batches(M.normalise(selection), n, batch)])
        want = in_rows[(present[in_rows] == 1) & (full[in_rows] > 10) & (in_rows >= 64)]
        kept = c.result_filter(res, pred, ["id", "v"])
        assert kept == len(want) == res.rows and res.n_batches == (len(want) + batch - 1) // batch and res.status()[0] == 0
        got_ids, got_vals = [], []
        for b in range(res.n_batches):
            a, v = res.batch(b, 0), res.batch(b, 1)
            assert a["length"] == v["length"] == min(batch, len(want) - b * batch)
            assert a["null_count"] == 0 and a["validity"] is None and v["null_count"] == 0 and v["validity"] is None
            got_ids.append(np.frombuffer(a["values"], dtype=np.int64))
            got_vals.append(np.frombuffer(v["values"], dtype=np.int64))
        assert np.array_equal(np.concatenate(got_ids), want) and np.array_equal(np.concatenate(got_vals), full[want])
        res.fetch()
        exported = pa.Table.from_batches([res.export_batch(b) for b in range(res.n_batches)])
        assert exported.column(0).to_pylist() == want.tolist() and exported.column(1).to_pylist() == full[want].tolist()
        with pytest.raises(capi.OrcGpuError) as e:  # once only
            c.result_filter(res, pred, ["id", "v"])
        assert e.value.code == 101
        res.free()
    # nulls that are kept keep their validity, with exact null counts per output batch
    staged = c.stage(n, streams, cols, batch_size=batch)
    res = c.decode([staged])[0]
    staged.free()
    kept = c.result_filter(res, P.or_([P.is_null("v"), P.lt("v", V.Int64(-40))]), ["id", "v"])
    want = ids[(present == 0) | (full < -40)]
    assert kept == len(want)
    for b in range(res.n_batches):
        v = res.batch(b, 1)
        rows = want[b * batch:(b + 1) * batch]
        assert v["null_count"] == int((present[rows] == 0).sum())
        bits = np.unpackbits(np.frombuffer(v["validity"], dtype=np.uint8), bitorder="little")[:len(rows)]
        assert np.array_equal(bits, present[rows])
    res.free()


def test_seeded_fuzz_against_the_model(tmpdir):
    path, table, rows = orc_file(tmpdir, 4097, "uncompressed")
    preds = FM.random_predicates(table, 200)
    partial = 0
    for k, pred in enumerate(preds):
        _, (seen, kept), _ = check(path, table, rows, pred, 1000, prefetch=2 if k % 2 else 0)
        partial += 0 < kept < 4097
    print("predicates that kept some but not all rows:", partial)
    assert partial >= 50
