"""ArrowWriter on the GPU (orcgpu_writer_*, orc_rust_amd.ArrowWriterBuilder): the whole file's bytes against the Python model of
the reference's writer (tests/writer_model.py, pinned by tests/test_writer_model.py), and every file read back by two readers --
pyarrow.orc (Apache ORC C++) and this project's ArrowReaderBuilder -- equal to what was written."""
import ctypes as C
import io

import numpy as np
import pyarrow as pa
import pyarrow.orc as po
import pytest

import gpu_util as G
import oracle_lib as O
import writer_model as WM
from orc_rust_amd import ArrowReaderBuilder, ArrowWriterBuilder, capi

pytestmark = pytest.mark.gpu

ALL_TYPES = [pa.bool_(), pa.int8(), pa.int16(), pa.int32(), pa.int64(), pa.float32(), pa.float64(), pa.string(), pa.large_string(),
             pa.binary(), pa.large_binary()]


def _column(t, n, rng, mode):
    """mode: "plain" (no validity buffer), "bitmap" (a validity buffer, no nulls), "nulls" """
    if t == pa.bool_():
        py = (rng.random(n) < 0.3).tolist()
    elif pa.types.is_integer(t):
        bits = t.bit_width
        lo, hi = -(1 << (bits - 3)), (1 << (bits - 3))  # (full-width deltas overflow N in the reference encoder)
        base = np.repeat(rng.integers(lo, hi, n // 6 + 2), rng.integers(1, 12, n // 6 + 2))[:n]
        if len(base) < n:
            base = np.concatenate([base, rng.integers(lo, hi, n - len(base))])
        base[n // 3: n // 2] = np.arange(n // 2 - n // 3) % (hi - 1)
        py = base.tolist()
    elif pa.types.is_floating(t):
        py = rng.standard_normal(n).astype(np.float32 if t == pa.float32() else np.float64).tolist()
    else:
        words = [b"", b"a", b"orc", b"\xff\x00zz", b"longer value here"]
        py = [words[i % 5] * (1 + i % 3) for i in rng.integers(0, 1000, n)]
        if pa.types.is_string(t) or pa.types.is_large_string(t):
            py = [x.decode("latin-1") for x in py]
    if mode == "plain":
        return pa.array(py, type=t)
    mask = rng.random(n) < 0.25 if mode == "nulls" else np.zeros(n, dtype=bool)
    arr = pa.array(py, type=t, mask=mask)
    if mode == "bitmap" and arr.buffers()[0] is None:
        bm = pa.py_buffer(np.packbits(np.ones(n, dtype=np.uint8), bitorder="little").tobytes())
        arr = pa.Array.from_buffers(t, n, [bm] + arr.buffers()[1:], null_count=-1)
    return arr


def _batch(n, rng, mode="nulls", types=ALL_TYPES):
    return pa.RecordBatch.from_arrays([_column(t, n, rng, mode) for t in types], names=["c%d" % i for i in range(len(types))])


def gpu_write(batches, schema=None, batch_size=1024, stripe_byte_size=64 << 20, flush_after=(), sink=None, ctx=None):
    schema = schema or batches[0].schema
    out = sink if sink is not None else io.BytesIO()
    w = ArrowWriterBuilder(out, schema, ctx=ctx or G.ctx()).with_batch_size(batch_size).with_stripe_byte_size(stripe_byte_size).try_build()
    for i, b in enumerate(batches):
        w.write(b)
        if i in flush_after:
            w.flush_stripe()
    w.close()
    rows, stats = w.stripe_rows(), w.stats()
    w.free()
    return (out.getvalue() if sink is None else None), rows, stats


def _plain_types(table):
    """The types the file reads back as: LargeUtf8 / LargeBinary are written as STRING / BINARY."""
    fields = []
    for f in table.schema:
        t = {pa.large_string(): pa.string(), pa.large_binary(): pa.binary()}.get(f.type, f.type)
        fields.append(pa.field(f.name, t))
    return table.cast(pa.schema(fields))


def check_readers(data, batches, schema=None):
    expect = _plain_types(pa.Table.from_batches(batches, schema=schema or batches[0].schema))
    got = po.ORCFile(io.BytesIO(data)).read()
    assert got.equals(expect), "pyarrow.orc read back something else"
    mine = list(ArrowReaderBuilder.try_new(data, ctx=G.ctx()).build())
    assert sum(b.num_rows for b in mine) == expect.num_rows
    if expect.num_rows:
        for i, f in enumerate(expect.schema):  # (values and nulls: the reader states a column without PRESENT as not nullable)
            got_col = pa.concat_arrays([b.column(i) for b in mine])
            assert got_col.equals(expect.column(i).combine_chunks()), "ArrowReaderBuilder read back something else in %s" % f.name


def check(batches, schema=None, flush_after=(), **kw):
    O.lib()
    want, want_rows = WM.write_model(batches, schema=schema, flush_after=flush_after, **kw)
    got, rows, stats = gpu_write(batches, schema=schema, flush_after=flush_after, **kw)
    assert rows == want_rows, (rows, want_rows)
    assert got == want, "file bytes differ from the model's (%d vs %d bytes)" % (len(got), len(want))
    check_readers(got, batches, schema)
    return rows, stats


@pytest.mark.parametrize("mode", ["plain", "bitmap", "nulls"])
def test_every_type_bytes(mode):
    rng = np.random.default_rng({"plain": 1, "bitmap": 2, "nulls": 3}[mode])
    check([_batch(2500, rng, mode)])


@pytest.mark.parametrize("batch_size", [1, 7, 1024, 8192])
@pytest.mark.parametrize("sbs", [256, 4096, 1 << 20, 64 << 20])
def test_batch_and_stripe_sizes(batch_size, sbs):
    rng = np.random.default_rng(batch_size * 31 + sbs)
    n = 600 if batch_size == 1 else 3000
    types = ALL_TYPES if batch_size != 1 else [pa.int8(), pa.int64(), pa.string(), pa.bool_(), pa.float32()]
    rows, _ = check([_batch(n, rng, "nulls", types)], batch_size=batch_size, stripe_byte_size=sbs)
    if sbs == 256 and batch_size < n:
        assert len(rows) > 1


def test_sliced_arrays():
    rng = np.random.default_rng(7)
    b = _batch(4000, rng, "nulls")
    check([b.slice(13, 2000), b.slice(1001, 1777), b.slice(3999, 1)], batch_size=100, stripe_byte_size=4096)


def test_many_uneven_and_empty_batches():
    rng = np.random.default_rng(8)
    schema = _batch(1, rng).schema
    empty = pa.RecordBatch.from_arrays([pa.array([], type=f.type) for f in schema], schema=schema)
    bs = [_batch(n, rng, ["plain", "nulls", "bitmap"][n % 3]) if n else empty for n in [0, 5, 1023, 1, 0, 2048, 333, 0, 64]]
    check(bs, schema=schema, batch_size=100, stripe_byte_size=2048)


def test_flush_between_writes():
    rng = np.random.default_rng(9)
    b1, b2 = _batch(700, rng, "plain"), _batch(300, rng, "plain")
    rows, _ = check([b1, b2, b2], flush_after=(0, 1), batch_size=256)
    assert rows == [700, 300, 300]
    # flush_stripe() with nothing pending: a stripe of 0 rows
    schema = b1.schema
    O.lib()
    m = WM.WriterModel(schema, 1024)
    m.write(b1)
    m.flush_stripe()
    m.flush_stripe()
    want = m.close()
    out = io.BytesIO()
    w = ArrowWriterBuilder(out, schema, ctx=G.ctx()).try_build()
    w.write(b1)
    w.flush_stripe()
    w.flush_stripe()
    w.close()
    assert w.stripe_rows() == [700, 0]
    w.free()
    assert out.getvalue() == want
    check_readers(out.getvalue(), [b1])


def test_sticky_present_across_stripes():
    rng = np.random.default_rng(10)
    types = [pa.int32(), pa.string(), pa.bool_(), pa.float64(), pa.int8()]
    plain, nullable = _batch(900, rng, "plain", types), _batch(400, rng, "nulls", types)
    rows, _ = check([plain, nullable, plain, plain], batch_size=64, stripe_byte_size=1024)
    assert len(rows) > 3


def test_runs_straddle_slices_and_cuts():
    """Long runs (fixed, delta, literal) across slice ends and stripe cuts."""
    n = 20000
    rng = np.random.default_rng(11)
    v = np.concatenate([np.full(5000, 42), np.arange(5000) * 3, rng.integers(-1 << 50, 1 << 50, 5000), np.repeat(rng.integers(0, 3, 2500), 2)])
    b8 = np.concatenate([np.full(5000, 1), rng.integers(-128, 128, 10000), np.repeat(rng.integers(-2, 2, 2500), 2)]).astype(np.int8)
    lens = np.concatenate([np.full(7000, 3), rng.integers(0, 40, 13000)])
    batch = pa.RecordBatch.from_pydict({"v": pa.array(v.astype(np.int64)), "b": pa.array(b8), "s": pa.array(["x" * int(k) for k in lens])})
    for bs, sbs in [(1000, 512), (333, 4096), (4096, 300)]:
        rows, _ = check([batch.slice(0, 7777), batch.slice(7777)], batch_size=bs, stripe_byte_size=sbs)
        assert len(rows) > 1


# ---- the reference's writer tests (arrow_writer.rs:297-535), restated -------------------------------------------------------

def test_reference_roundtrip_write():
    b = pa.RecordBatch.from_pydict({
        "f32": pa.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0], pa.float32()), "f64": pa.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0]),
        "int8": pa.array([0, 1, 2, 3, 4, 5, 6], pa.int8()), "int16": pa.array([0, 1, 2, 3, 4, 5, 6], pa.int16()),
        "int32": pa.array([0, 1, 2, 3, 4, 5, 6], pa.int32()), "int64": pa.array([0, 1, 2, 3, 4, 5, 6], pa.int64()),
        "utf8": pa.array(["Hello", "there", "楡井希実", "💯", "ÃÃÃ", "ÇÇÇ", "ÈÈÈ"]),
        "binary": pa.array([b"", b"123", b"\x00\x01", b"abc", b"\xff" * 3, b"x", b"yy"], pa.binary()),
        "bool": pa.array([True, False, True, False, True, False, True]),
    })
    check([b, b])


def test_reference_roundtrip_large_types():
    b = pa.RecordBatch.from_pydict({"large_utf8": pa.array(["Hello", "there", "楡井希実", "💯", "ÃÃÃ", "ÇÇÇ", "ÈÈÈ"], pa.large_string()),
                                    "large_binary": pa.array([b"", b"123", b"\x00\x01", b"abc", b"x", b"yy", b"zzz"], pa.large_binary())})
    data, _, _ = gpu_write([b, b])
    got = po.ORCFile(io.BytesIO(data)).read()
    assert got.schema.field("large_utf8").type == pa.string() and got.schema.field("large_binary").type == pa.binary()
    check([b, b])


def test_reference_write_small_stripes():
    n = 1_000_000
    b = pa.RecordBatch.from_pydict({"x": pa.array(np.arange(n, dtype=np.int64))})
    rows, _ = check([b], stripe_byte_size=256)
    assert len(rows) > 1 and sum(rows) == n


def test_reference_inconsistent_null_buffers():
    schema = pa.schema([("x", pa.int64()), ("s", pa.string())])
    b1 = pa.RecordBatch.from_pydict({"x": pa.array([1, 2, 3], pa.int64()), "s": pa.array(["a", "b", "c"])}, schema=schema)
    b2 = pa.RecordBatch.from_pydict({"x": pa.array([None, 5, None], pa.int64()), "s": pa.array([None, "e", None])}, schema=schema)
    check([b1, b2])


def test_reference_empty_null_buffers():
    """A validity buffer with no nulls: the file holds a PRESENT stream, the column reads back without nulls."""
    n = 5
    bm = pa.py_buffer(bytes([0xFF]))
    x = pa.Array.from_buffers(pa.int64(), n, [bm, pa.array(np.arange(n, dtype=np.int64)).buffers()[1]], null_count=-1)
    b = pa.RecordBatch.from_arrays([x], names=["x"])
    assert b.column(0).buffers()[0] is not None
    check([b])
    data, _, _ = gpu_write([b])
    # the stripe footer lists a PRESENT stream (kind 0) of column 1
    f = po.ORCFile(io.BytesIO(data))
    assert f.read().column(0).null_count == 0
    tail = data[3:]
    assert bytes([0x0A, 0x06, 0x08, 0x00, 0x10, 0x01, 0x18]) in tail


# ---- device input -------------------------------------------------------------------------------------------------------------

class _ArrowArray(C.Structure):
    pass


_ArrowArray._fields_ = [("length", C.c_int64), ("null_count", C.c_int64), ("offset", C.c_int64), ("n_buffers", C.c_int64),
                        ("n_children", C.c_int64), ("buffers", C.POINTER(C.c_void_p)), ("children", C.POINTER(C.POINTER(_ArrowArray))),
                        ("dictionary", C.c_void_p), ("release", C.c_void_p), ("private_data", C.c_void_p)]


def test_device_batch_from_the_reader():
    """A batch the GPU decoder produced, written from its device buffers (ORCGPU_ENC_ON_DEVICE): the same bytes as from the host."""
    from orc_rust_amd import gen
    rng = np.random.default_rng(12)
    n = 20000
    present = (rng.random(n) > 0.15).astype(np.uint8)
    k = int(present.sum())
    vals = np.concatenate([np.repeat(rng.integers(0, 50, k // 8 + 1), 4)[: k // 2], rng.integers(-1 << 40, 1 << 40, k - k // 2)]).astype(np.int64)
    cols = [{"column_id": 1, "orc_type": 4, "encoding": 2}]
    streams = [(1, 0, gen.boolean(present)), (1, 1, gen.rle2(vals, signed=True))]
    res = G.gpu_decode(n, cols, streams, batch_size=8192)
    assert res.status()[0] == 0
    v = res.view(1, 0)  # the second batch: rows 8192 .. 16383
    host = res.batch(1, 0)
    m = v.length
    valid = np.unpackbits(np.frombuffer(host["validity"], dtype=np.uint8), bitorder="little")[:m].astype(bool) if v.validity else np.ones(m, bool)
    xs = np.frombuffer(host["values"], dtype=np.int64)[:m]
    hb = pa.RecordBatch.from_arrays([pa.array(xs, mask=~valid)], names=["x"])
    want, _, _ = gpu_write([hb], batch_size=1000, stripe_byte_size=2048)
    # the same rows from the device buffers
    child = _ArrowArray()
    cbufs = (C.c_void_p * 2)(v.validity, v.values)
    child.length, child.null_count, child.offset, child.n_buffers, child.n_children, child.buffers = m, v.null_count, 0, 2, 0, cbufs
    root = _ArrowArray()
    rbufs = (C.c_void_p * 1)(None)
    kids = (C.POINTER(_ArrowArray) * 1)(C.pointer(child))
    root.length, root.null_count, root.offset, root.n_buffers, root.n_children, root.buffers, root.children = m, 0, 0, 1, 1, rbufs, kids
    out = io.BytesIO()
    w = ArrowWriterBuilder(out, hb.schema, ctx=G.ctx()).with_batch_size(1000).with_stripe_byte_size(2048).try_build()
    sbuf = (C.c_uint8 * 72)()
    hb.schema._export_to_c(C.addressof(sbuf))
    try:
        w.write_c(C.addressof(sbuf), C.addressof(root), capi.ENC_ON_DEVICE)
    finally:
        rel = C.cast(C.addressof(sbuf) + 56, C.POINTER(C.CFUNCTYPE(None, C.c_void_p)))[0]
        rel(C.addressof(sbuf))
    w.close()
    w.free()
    res.free()
    assert out.getvalue() == want
    check_readers(want, [hb])


# ---- errors -------------------------------------------------------------------------------------------------------------------

def test_errors():
    schema = pa.schema([("x", pa.int64())])
    w = ArrowWriterBuilder(io.BytesIO(), schema, ctx=G.ctx()).try_build()
    other = pa.RecordBatch.from_pydict({"y": pa.array([1], pa.int64())})
    with pytest.raises(capi.OrcGpuError) as e:
        w.write(other)
    assert e.value.code == 10  # ORCGPU_UNEXPECTED
    nonnull = pa.RecordBatch.from_arrays([pa.array([1], pa.int64())], schema=pa.schema([pa.field("x", pa.int64(), nullable=False)]))
    with pytest.raises(capi.OrcGpuError) as e:
        w.write(nonnull)
    assert e.value.code == 10
    w.close()
    with pytest.raises(capi.OrcGpuError) as e:
        w.write(pa.RecordBatch.from_pydict({"x": pa.array([1], pa.int64())}))
    assert e.value.code == 101  # ORCGPU_INVALID_ARGUMENT
    w.free()
    with pytest.raises(capi.OrcGpuError) as e:
        ArrowWriterBuilder(io.BytesIO(), pa.schema([("d", pa.date32())]), ctx=G.ctx()).try_build()
    assert e.value.code == 7  # ORCGPU_UNSUPPORTED


def test_close_without_rows_and_file_sink(tmp_path):
    schema = pa.schema([("x", pa.int64()), ("s", pa.string())])
    data, rows, _ = gpu_write([], schema=schema)
    assert rows == [] and data == WM.write_model([], schema=schema)[0]
    f = po.ORCFile(io.BytesIO(data))
    assert f.nrows == 0 and f.nstripes == 0
    b = pa.RecordBatch.from_pydict({"x": pa.array([1, None, 3], pa.int64()), "s": pa.array(["a", "bb", None])}, schema=schema)
    p = tmp_path / "w.orc"
    w = ArrowWriterBuilder(str(p), schema, ctx=G.ctx()).try_build()
    w.write(b)
    w.write(b)
    w.close()
    w.free()
    assert p.read_bytes() == WM.write_model([b, b])[0]


# ---- scale ---------------------------------------------------------------------------------------------------------------------

def _one(a):
    return a.combine_chunks() if isinstance(a, pa.ChunkedArray) else a


def _lineitem(n, rng):
    return pa.RecordBatch.from_pydict({k: _one(v) for k, v in {
        "l_orderkey": pa.array(np.repeat(np.arange(n // 4 + 1, dtype=np.int64) * 4, 4)[:n]),
        "l_partkey": pa.array(rng.integers(1, 200000, n).astype(np.int64)),
        "l_suppkey": pa.array(rng.integers(1, 10000, n).astype(np.int64)),
        "l_linenumber": pa.array((np.arange(n) % 7 + 1).astype(np.int32)),
        "l_quantity": pa.array(rng.integers(1, 51, n).astype(np.float64)),
        "l_extendedprice": pa.array(np.round(rng.random(n) * 100000, 2)),
        "l_discount": pa.array(rng.integers(0, 11, n) / 100.0),
        "l_tax": pa.array(rng.integers(0, 9, n) / 100.0),
        "l_returnflag": pa.array(np.array(["A", "N", "R"])[rng.integers(0, 3, n)]),
        "l_linestatus": pa.array(np.array(["O", "F"])[rng.integers(0, 2, n)]),
        "l_shipdate": pa.array(rng.integers(8000, 10600, n).astype(np.int32)),
        "l_commitdate": pa.array(rng.integers(8000, 10600, n).astype(np.int32)),
        "l_receiptdate": pa.array(rng.integers(8000, 10600, n).astype(np.int32)),
        "l_shipinstruct": pa.array(np.array(["DELIVER IN PERSON", "COLLECT COD", "NONE", "TAKE BACK RETURN"])[rng.integers(0, 4, n)]),
        "l_shipmode": pa.array(np.array(["AIR", "MAIL", "SHIP", "TRUCK", "RAIL", "FOB", "REG AIR"])[rng.integers(0, 7, n)]),
        "l_comment": pa.array(["c%x" % x for x in rng.integers(0, 1 << 40, n)]),
    }.items()})


def test_scale_lineitem():
    rng = np.random.default_rng(13)
    n = 2_000_000
    b = _lineitem(n, rng)
    batches = [b.slice(i, 250_000) for i in range(0, n, 250_000)]
    for sbs in [64 << 20, 4 << 20]:
        data, rows, stats = gpu_write(batches, stripe_byte_size=sbs)
        assert sum(rows) == n
        assert po.ORCFile(io.BytesIO(data)).read().equals(pa.Table.from_batches(batches))
        if sbs == 4 << 20:
            assert len(rows) > 3
    # the cut points against the model on a share small enough for it
    part = [b.slice(0, 150_000)]
    check(part, stripe_byte_size=1 << 20)


# ---- host round trips ------------------------------------------------------------------------------------------------------------

def _round_trips_per_write_and_stripe(types, sbs=64 << 20):
    rng = np.random.default_rng(14)
    b = _batch(20000, rng, "nulls", types)
    w = ArrowWriterBuilder(io.BytesIO(), b.schema, ctx=G.ctx()).with_stripe_byte_size(sbs).try_build()
    w.write(b)
    w.flush_stripe()  # (the first stripe grows the buffers)
    s0 = w.stats()
    for _ in range(3):
        w.write(b)
        w.flush_stripe()
    s1 = w.stats()
    w.close()
    w.free()
    stripes = s1["stripes"] - s0["stripes"]
    return (s1["round_trips"] - s0["round_trips"]) / 3, (s1["stripe_round_trips"] - s0["stripe_round_trips"]) / stripes


def test_round_trips_do_not_grow_with_the_columns():
    """orcgpu_writer_stats: the host round trips of a write and its stripe are the same for 2 columns and for 16."""
    two = [pa.int64(), pa.string()]
    sixteen = [pa.int64(), pa.int32(), pa.int16(), pa.int8(), pa.bool_(), pa.float32(), pa.float64(), pa.string(), pa.large_string(),
               pa.binary(), pa.large_binary(), pa.int64(), pa.int32(), pa.string(), pa.int8(), pa.bool_()]
    a, b = _round_trips_per_write_and_stripe(two), _round_trips_per_write_and_stripe(sixteen)
    assert a == b, (a, b)
    assert a[1] <= 3, a
    # stripes cut by size inside the writes: the same per stripe
    a, b = _round_trips_per_write_and_stripe(two, 64 << 10), _round_trips_per_write_and_stripe(sixteen, 64 << 10)
    assert a[1] == b[1] <= 3, (a, b)


# ---- device input of every type ------------------------------------------------------------------------------------------------

class _DeviceBatch:
    """A pyarrow batch's buffers copied to device memory, as an Arrow C struct array of device pointers (offsets kept)."""

    def __init__(self, batch):
        self.hip = C.CDLL("libamdhip64.so")
        self.ptrs, self.keep, kids = [], [], []
        for col in batch.columns:
            bufs = []
            for buf in col.buffers():
                if buf is None:
                    bufs.append(None)
                    continue
                p = C.c_void_p()
                assert self.hip.hipMalloc(C.byref(p), C.c_size_t(max(1, buf.size))) == 0
                assert self.hip.hipMemcpy(p, C.c_void_p(buf.address), C.c_size_t(buf.size), 1) == 0  # host -> device
                self.ptrs.append(p)
                bufs.append(p.value)
            arr = _ArrowArray()
            cb = (C.c_void_p * len(bufs))(*bufs)
            arr.length, arr.null_count, arr.offset, arr.n_buffers, arr.n_children, arr.buffers = len(col), col.null_count, col.offset, len(bufs), 0, cb
            self.keep += [arr, cb]
            kids.append(C.pointer(arr))
        self.kids = (C.POINTER(_ArrowArray) * max(1, len(kids)))(*kids)
        self.rbufs = (C.c_void_p * 1)(None)
        self.root = _ArrowArray()
        r = self.root
        r.length, r.null_count, r.offset, r.n_buffers, r.n_children, r.buffers, r.children = batch.num_rows, 0, 0, 1, len(kids), self.rbufs, self.kids

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


def test_device_batches_of_every_type():
    """Every type, with nulls, bit offsets (sliced arrays) and string offsets that do not start at 0, from device buffers
    (ORCGPU_ENC_ON_DEVICE): the same file as from the host."""
    rng = np.random.default_rng(15)
    full = _batch(5000, rng, "nulls")
    batches = [full.slice(3, 1500), full.slice(1777, 2000), _batch(900, rng, "plain")]
    batches[2] = pa.RecordBatch.from_arrays(batches[2].columns, schema=full.schema)
    want, want_rows, _ = gpu_write(batches, batch_size=300, stripe_byte_size=8192)
    dev = [_DeviceBatch(b) for b in batches]
    out = io.BytesIO()
    w = ArrowWriterBuilder(out, full.schema, ctx=G.ctx()).with_batch_size(300).with_stripe_byte_size(8192).try_build()
    sbuf = (C.c_uint8 * 72)()
    full.schema._export_to_c(C.addressof(sbuf))
    try:
        for d in dev:
            w.write_c(C.addressof(sbuf), C.addressof(d.root), capi.ENC_ON_DEVICE)
    finally:
        C.cast(C.addressof(sbuf) + 56, C.POINTER(C.CFUNCTYPE(None, C.c_void_p)))[0](C.addressof(sbuf))
    w.close()
    rows = w.stripe_rows()
    w.free()
    for d in dev:
        d.free()
    assert rows == want_rows and len(rows) > 1
    assert out.getvalue() == want
    check_readers(want, batches)


def test_failed_write_leaves_the_writer_failed():
    schema = pa.schema([("x", pa.int64()), ("s", pa.string())])
    good = pa.RecordBatch.from_pydict({"x": pa.array([1, 2], pa.int64()), "s": pa.array(["a", "b"])}, schema=schema)
    # offsets that go down: rejected before anything changes, the writer goes on
    bad_s = pa.Array.from_buffers(pa.string(), 2, [None, pa.py_buffer(np.array([0, 5, 1], dtype=np.int32).tobytes()), pa.py_buffer(b"abcde")])
    bad = pa.RecordBatch.from_arrays([pa.array([None, 4], pa.int64()), bad_s], schema=schema)
    out = io.BytesIO()
    w = ArrowWriterBuilder(out, schema, ctx=G.ctx()).try_build()
    w.write(good)
    with pytest.raises(capi.OrcGpuError) as e:
        w.write(bad)
    assert e.value.code == 101
    w.write(good)
    w.close()
    w.free()
    assert out.getvalue() == WM.write_model([good, good])[0]
