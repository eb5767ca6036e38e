"""ArrowWriter with a row index (orcgpu_writer_set_row_index, ArrowWriterBuilder.with_row_index_stride): ROW_INDEX streams,
the Metadata section and Footer.statistics, computed on the GPU.

- the indexed file has the stripes, rows and data streams of the same writes without an index;
- every group's, stripe's and the file's statistics are tests/index_model.py's;
- pyarrow and ArrowReaderBuilder read it back; seeking to a group by its positions reads that group alone;
- predicates prune the row groups the statistics rule out."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.orc as po
import pytest

import gpu_util as G
import index_model as IM
import oracle_lib as O
from orcfile import DATA, LENGTH, PRESENT, ROW_INDEX, OrcFile
from orc_rust_amd import ArrowReaderBuilder, ArrowWriterBuilder
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
from test_gpu_writer import ALL_TYPES, _batch, _lineitem, _plain_types

pytestmark = pytest.mark.gpu


def write(batches, stride=0, comp=None, batch_size=1024, sbs=64 << 20, flush_after=(), device=False):
    out = io.BytesIO()
    b = ArrowWriterBuilder(out, batches[0].schema, ctx=G.ctx()).with_batch_size(batch_size).with_stripe_byte_size(sbs)
    if comp:
        b = b.with_compression(comp)
    if stride:
        b = b.with_row_index_stride(stride)
    w = b.try_build()
    for i, x in enumerate(batches):
        w.write(x)
        if i in flush_after:
            w.flush_stripe()
    w.close()
    rows, stats = w.stripe_rows(), w.stats()
    w.free()
    return out.getvalue(), rows, stats


def data_streams(of):
    return [[(k, c, bytes(s.streams[(c, k)])) for k, c, _ in s.stream_list if k != ROW_INDEX] for s in of.stripes]


def check_index(data, table, rows, stride):
    """the file's index and statistics against the model, field for field"""
    O.lib()
    of = OrcFile(data)
    assert of.row_index_stride == stride
    assert [s.number_of_rows for s in of.stripes] == rows
    groups, stripes, whole = IM.model_groups(table, rows, stride)
    ncol = table.num_columns + 1
    cols = [table.column(i).combine_chunks() for i in range(table.num_columns)]
    at = 0
    for si, s in enumerate(of.stripes):
        kinds = [k for k, _, _ in s.stream_list]
        assert kinds[:ncol] == [ROW_INDEX] * ncol and ROW_INDEX not in kinds[ncol:]
        assert [c for _, c, _ in s.stream_list[:ncol]] == list(range(ncol))
        assert s.index_length == sum(l for _, _, l in s.stream_list[:ncol])
        for col in range(ncol):
            entries = IM.row_index_entries(of, s, col)
            assert len(entries) == len(groups[si])
            want_pos = []
            if col:
                raws = None
                if of.compression:
                    names = {PRESENT: "PRESENT", DATA: "DATA", LENGTH: "LENGTH"}
                    raws = {names[k]: bytes(v) for (c, k), v in s.streams.items() if c == col and k in names}
                want_pos = IM.model_positions(cols[col - 1].slice(at, s.number_of_rows), (col, PRESENT) in s.streams, stride, raws, of.block_size)
            for g, (pos, st) in enumerate(entries):
                assert IM.same_stats(st, groups[si][g][col]), (si, g, col, st, groups[si][g][col])
                assert pos == (want_pos[g] if col else []), (si, g, col, pos, want_pos[g] if col else [])
        at += s.number_of_rows
    fstats, sstats = IM.file_statistics(of)
    assert len(sstats) == len(of.stripes)
    for si, ss in enumerate(sstats):
        assert len(ss) == ncol
        for col in range(ncol):
            assert IM.same_stats(ss[col], stripes[si][col]), (si, col, ss[col], stripes[si][col])
    assert len(fstats) == ncol
    for col in range(ncol):
        assert IM.same_stats(fstats[col], whole[col]), (col, fstats[col], whole[col])
    f = po.ORCFile(io.BytesIO(data))
    assert f.nstripe_statistics == f.nstripes
    got, want = f.read(), _plain_types(table)
    for name in want.column_names:  # (NaN: equal to itself here)
        a, b = got.column(name).combine_chunks(), want.column(name).combine_chunks()
        if pa.types.is_floating(b.type):
            assert a.is_null().equals(b.is_null())
            np.testing.assert_array_equal(a.fill_null(0).to_numpy(), b.fill_null(0).to_numpy())
        else:
            assert a.equals(b), name
    # ArrowReaderBuilder reads it unchanged
    mine = list(ArrowReaderBuilder.try_new(data, ctx=G.ctx()).build())
    assert sum(x.num_rows for x in mine) == want.num_rows
    if want.num_rows:
        for i, name in enumerate(want.column_names):
            a, b = pa.concat_arrays([x.column(i) for x in mine]), want.column(name).combine_chunks()
            if pa.types.is_floating(b.type):
                assert a.is_null().equals(b.is_null())
                np.testing.assert_array_equal(a.fill_null(0).to_numpy(), b.fill_null(0).to_numpy())
            else:
                assert a.equals(b), name


@pytest.mark.parametrize("comp", [None, "snappy", "lz4"])
@pytest.mark.parametrize("stride", [1, 7, 8, 1001, 10000])
def test_invariant_and_model(comp, stride):
    rng = np.random.default_rng(stride)
    n = 3000 if stride < 8 else 23000
    batches = [_batch(n, rng, "nulls"), _batch(n // 3 + 5, rng, "plain")]
    plain, rows0, _ = write(batches, 0, comp, sbs=256 << 10, flush_after=(0,))
    data, rows, _ = write(batches, stride, comp, sbs=256 << 10, flush_after=(0,))
    assert rows == rows0 and len(rows) >= 2
    assert data_streams(OrcFile(data)) == data_streams(OrcFile(plain))
    table = pa.Table.from_batches(batches)
    check_index(data, table, rows, stride)
    again, _, _ = write(batches, stride, comp, sbs=256 << 10, flush_after=(0,))
    assert again == data


def test_default_is_unchanged():
    rng = np.random.default_rng(3)
    b = [_batch(5000, rng)]
    a, _, _ = write(b)
    c, _, _ = write(b, 0)
    assert a == c
    assert OrcFile(a).row_index_stride is None


def test_edges():
    rng = np.random.default_rng(5)
    n = 4100
    i64 = np.full(n, (1 << 63) - 1, dtype=np.int64)
    i64[::3] = -(1 << 63)
    f = rng.standard_normal(n)
    f[:5] = [np.inf, -np.inf, -0.0, 0.0, 1.0]
    f[2000] = np.nan
    long = "a" + "é" * 600 + "x"  # (1202 bytes: byte 1024 is the second byte of a character, the bound backs off to 1023)
    top = "z" + "\U0010ffff" * 300  # (the maximum: its bound's last characters have no successor, "{" is the upper bound)
    strs = ["", "a", long, long + "z", "\U0010fffe" * 300, top] + ["s%d" % i for i in range(n - 6)]
    cols = {
        "i64": pa.array(i64),
        "i8": pa.array(rng.integers(-128, 128, n).astype(np.int8), mask=rng.random(n) < 0.5),
        "i16": pa.array(rng.integers(-9, 9, n).astype(np.int16), mask=np.ones(n, bool)),
        "i32": pa.array(rng.integers(-9, 9, n).astype(np.int32)),
        "f64": pa.array(f),
        "f32": pa.array(f.astype(np.float32), mask=np.arange(n) < 1000),
        "s": pa.array(strs),
        "ls": pa.array(strs[::-1], type=pa.large_string()),
        "bin": pa.array([x.encode() for x in strs], type=pa.binary()),
        "lbin": pa.array([x.encode() for x in strs], type=pa.large_binary(), mask=rng.random(n) < 0.5),
        "b": pa.array(rng.random(n) < 0.5, mask=rng.random(n) < 0.1),
    }
    batch = pa.RecordBatch.from_pydict(cols)
    for comp in [None, "lz4"]:
        batches = [batch.slice(0, 1234), batch.slice(1234)]
        data, rows, _ = write(batches, 1000, comp, batch_size=333, flush_after=(0, 1))
        check_index(data, pa.Table.from_batches(batches), rows, 1000)


def test_zero_row_stripes():
    rng = np.random.default_rng(6)
    b = _batch(3000, rng)
    out = io.BytesIO()
    w = ArrowWriterBuilder(out, b.schema, ctx=G.ctx()).with_row_index_stride(1000).try_build()
    w.flush_stripe()
    w.write(b)
    w.flush_stripe()
    w.flush_stripe()
    w.close()
    rows = w.stripe_rows()
    w.free()
    assert 0 in rows
    check_index(out.getvalue(), pa.Table.from_batches([b]), rows, 1000)


def test_round_trips_unchanged():
    rng = np.random.default_rng(7)
    b = _batch(20000, rng)

    def trips(stride):
        w = ArrowWriterBuilder(io.BytesIO(), b.schema, ctx=G.ctx()).with_row_index_stride(stride).try_build()
        w.write(b)
        w.flush_stripe()
        s0 = w.stats()
        for _ in range(3):
            w.write(b)
            w.flush_stripe()
        s1 = w.stats()
        w.close()
        w.free()
        return s1["stripe_round_trips"] - s0["stripe_round_trips"], s1["round_trips"] - s0["round_trips"]

    assert trips(0) == trips(10000) == trips(7)


def same_values(got, want):
    """equal column by column (the reader states a column without PRESENT as not nullable)"""
    assert got.num_rows == want.num_rows and got.column_names == want.column_names
    for i in range(want.num_columns):
        a, b = got.column(i).combine_chunks(), want.column(i).combine_chunks()
        if pa.types.is_floating(b.type):  # (NaN equal to itself)
            if not a.is_null().equals(b.is_null()):
                return False
            x, y = a.fill_null(0).to_numpy(), b.fill_null(0).to_numpy()
            if not np.array_equal(x, y, equal_nan=True):
                return False
        elif not a.equals(b):
            return False
    return True


def _read(data, predicate=None, selection=None, batch_size=8192):
    # (a selected run longer than batch_size runs on to the stripe's end, as the reference's selection does: the tests keep runs
    # that fit one batch, or read with batches as large as the kept rows)
    b = ArrowReaderBuilder.try_new(data, G.ctx()).with_batch_size(batch_size)
    if predicate is not None:
        b = b.with_predicate(predicate)
    if selection is not None:
        b = b.with_row_selection(selection)
    r = b.build()
    out = list(r)
    groups = r.row_groups()
    r.close()
    if not out:
        return None, groups
    # (batches of one file may state a column nullable or not: a piece without nulls has no PRESENT)
    names = out[0].schema.names
    return pa.table({n: pa.concat_arrays([x.column(i) for x in out]) for i, n in enumerate(names)}), groups


@pytest.mark.parametrize("comp", [None, "snappy"])
def test_seek_each_group(comp):
    rng = np.random.default_rng(8)
    n, S = 20000, 4096
    cols = {
        "i": pa.array(rng.integers(0, 50, n), mask=rng.random(n) < 0.3),
        "s": pa.array(["v%d" % x for x in rng.integers(0, 9999, n)], mask=rng.random(n) < 0.2),
        "f": pa.array(rng.standard_normal(n)),
        "l": pa.array(np.repeat(np.arange(n // 7 + 1), 7)[:n].astype(np.int64)),
    }
    batch = pa.RecordBatch.from_pydict(cols)
    data, rows, _ = write([batch], S, comp)
    assert rows == [n]
    whole = po.ORCFile(io.BytesIO(data)).read()
    assert ArrowReaderBuilder.try_new(data, G.ctx()).build() is not None
    G_ = (n + S - 1) // S
    for g in range(G_):
        lo, hi = g * S, min(n, (g + 1) * S)
        sel = ([(lo, True)] if lo else []) + [(hi - lo, False)] + ([(n - hi, True)] if hi < n else [])
        got, groups = _read(data, selection=sel)
        assert groups == (1, G_), (g, groups)
        assert same_values(got, whole.slice(lo, hi - lo)), g


@pytest.mark.parametrize("ncols", [4, 16])
def test_pushdown_lineitem(ncols):
    """the test that fails without the index: a file sorted on l_orderkey, read with l_orderkey < X, reads the groups the
    statistics keep and no others"""
    rng = np.random.default_rng(9)
    n, S = 120000, 10000
    b = _lineitem(n, rng)
    b = pa.RecordBatch.from_arrays(b.columns[:ncols], names=b.schema.names[:ncols])
    data, rows, _ = write([b], S, None)
    whole = po.ORCFile(io.BytesIO(data)).read()
    keys = whole.column("l_orderkey").to_numpy()
    for op, X, batch_size in [("lt", 4 * 25000 + 2, n), ("lt", 4 * 1500 + 1, S), ("gte", 110000, 8192), ("gte", 95001, n)]:
        lt = op == "lt"
        got, groups = _read(data, predicate=(P.lt if lt else P.gte)("l_orderkey", V.Int64(X)), batch_size=batch_size)
        lo, hi = keys[::S], keys[S - 1::S]
        want_groups = [g for g in range(n // S) if (lo[g] < X if lt else hi[g] >= X)]
        assert groups == (len(want_groups), n // S), (X, groups)
        assert 0 < len(want_groups) < n // S
        kept = pa.concat_tables([whole.slice(g * S, S) for g in want_groups])
        assert same_values(got, kept)
        match = keys < X if lt else keys >= X
        col = got.column("l_orderkey").to_numpy()
        assert ((col < X) if lt else (col >= X)).sum() == match.sum()


def test_pushdown_other_types():
    rng = np.random.default_rng(10)
    n, S = 40000, 8000
    s = np.array(["k%05d" % i for i in range(n)])
    f = np.arange(n, dtype=np.float64)
    f_nan = f.copy()
    f_nan[n - 3] = np.nan
    flag = np.zeros(n, bool)
    flag[S * 2: S * 2 + 10] = True
    nulls = np.zeros(n, bool)
    nulls[S * 4 + 1] = True
    b = pa.RecordBatch.from_pydict({"s": pa.array(s), "f": pa.array(f), "fn": pa.array(f_nan), "flag": pa.array(flag),
                                    "x": pa.array(np.arange(n), mask=nulls)})
    data, rows, _ = write([b], S, "lz4")
    whole = po.ORCFile(io.BytesIO(data)).read()
    G_ = n // S

    def check(pred, keep):
        got, groups = _read(data, predicate=pred)
        assert groups == (len(keep), G_), (groups, keep)
        assert same_values(got, pa.concat_tables([whole.slice(g * S, S) for g in keep]))

    check(P.lt("s", V.Utf8("k08000")), [0])
    check(P.gte("f", V.Float64(float(n - S))), [G_ - 1])
    check(P.lt("fn", V.Float64(1.0)), list(range(G_)))  # (NaN: no DoubleStatistics, nothing pruned)
    check(P.eq("flag", V.Boolean(True)), [2])
    check(P.is_null("x"), [4])


def test_device_input():
    """ORCGPU_ENC_ON_DEVICE: the same file as from the host, groups and stripes crossed inside the write"""
    import ctypes as C
    from orc_rust_amd import capi
    from test_gpu_writer import _ArrowArray
    hip = C.CDLL("libamdhip64.so")
    rng = np.random.default_rng(11)
    n = 9000
    xs = rng.integers(-50, 100, n).astype(np.int64)
    fs = rng.standard_normal(n)
    hb = pa.RecordBatch.from_arrays([pa.array(xs), pa.array(fs)], names=["x", "f"])
    want, rows, _ = write([hb], 1000, batch_size=700, sbs=8192)
    assert len(rows) > 1
    ptrs, keep, kids = [], [], []
    for a in (xs, fs):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0  # hipMemcpyHostToDevice
        ptrs.append(p)
        arr = _ArrowArray()
        bufs = (C.c_void_p * 2)(None, p.value)
        arr.length, arr.null_count, arr.offset, arr.n_buffers, arr.n_children, arr.buffers = n, 0, 0, 2, 0, bufs
        keep += [arr, bufs]
        kids.append(C.pointer(arr))
    root = _ArrowArray()
    rbufs = (C.c_void_p * 1)(None)
    kid_arr = (C.POINTER(_ArrowArray) * 2)(*kids)
    root.length, root.null_count, root.offset, root.n_buffers, root.n_children, root.buffers, root.children = n, 0, 0, 1, 2, rbufs, kid_arr
    out = io.BytesIO()
    w = ArrowWriterBuilder(out, hb.schema, ctx=G.ctx()).with_batch_size(700).with_stripe_byte_size(8192).with_row_index_stride(1000).try_build()
    sbuf = (C.c_uint8 * 72)()
    hb.schema._export_to_c(C.addressof(sbuf))
    try:
        w.write_c(C.addressof(sbuf), C.addressof(root), capi.ENC_ON_DEVICE)
    finally:
        rel = C.cast(C.addressof(sbuf) + 56, C.POINTER(C.CFUNCTYPE(None, C.c_void_p)))[0]
        rel(C.addressof(sbuf))
    w.close()
    w.free()
    for p in ptrs:
        hip.hipFree(p)
    assert out.getvalue() == want
    check_index(want, pa.Table.from_batches([hb]), rows, 1000)
