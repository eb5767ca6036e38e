"""Device-resident batches on the GPU: ArrowReaderBuilder.with_device_output() hands out the decoder's own HBM buffers as torch
tensors (orcgpu_reader_next_batch_device, orcgpu_device_array_dlpack), and ArrowWriter.write_device() takes them back.  The
yardstick throughout is the host path of the same reader options: the batches must be the same, index by index."""
import ctypes as C
import gc
import io
import os

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import arrow_util as A
import orcfile
from orc_rust_amd import capi
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.arrow_writer import ArrowWriterBuilder
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

pytestmark = pytest.mark.gpu

FILES = ["alltypes.none.orc", "alltypes.zstd.orc", "decimal.orc", "pyarrow_timestamps.orc", "string_dict.orc", "long_bool.orc",
         "nulls-at-end-snappy.orc", "lineitem_8k.zstd.orc", "TestOrcFile.emptyFile.orc"]
BATCH_SIZES = (1000, 8192)
UNPACK_SIZES = (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 65537)
UNSUPPORTED, INVALID, END_OF_FILE = 7, 101, 110
_CTX = {}


def ctx(which=0):
    """which = 1: a second context on the same device (a writer beside a reader that reads ahead)"""
    if which not in _CTX:
        _CTX[which] = capi.Context(0)
    return _CTX[which]


def builder(source, batch_size=1000, device=False, prefetch=2, **opts):
    b = ArrowReaderBuilder.try_new(source, ctx()).with_batch_size(batch_size).with_prefetch(prefetch)
    if opts.get("projection") is not None:
        b = b.with_projection(opts["projection"])
    if opts.get("selection") is not None:
        b = b.with_row_selection(opts["selection"])
    if opts.get("predicate") is not None:
        b = b.with_predicate(opts["predicate"])
    if opts.get("row_filter") is not None:
        b = b.with_row_filter(opts["row_filter"], prune=opts.get("prune", True))
    return b.with_device_output() if device else b


def host_bits(buf, n):
    return np.unpackbits(np.frombuffer(buf, dtype=np.uint8), bitorder="little")[:n].astype(bool)


def assert_same_batches(source, batch_size, prefetch=2, **opts):
    """Every device batch, copied back, is the host reader's batch of the same index; its unpacked validity and Boolean tensors are
    the bits of the host buffers.  Returns the number of batches."""
    rh = builder(source, batch_size, False, prefetch, **opts).build()
    want = list(rh)
    rh.close()
    rd = builder(source, batch_size, True, prefetch, **opts).build()
    count = 0
    for k, db in enumerate(rd):
        assert k < len(want), (k, len(want))
        hb = want[k]
        got = db.to_pyarrow()
        assert got.schema.equals(hb.schema, check_metadata=True), (k, got.schema, hb.schema)
        assert db.schema.equals(hb.schema), k
        got.validate(full=True)
        assert got.equals(hb), k
        assert db.num_rows == hb.num_rows
        for i in range(hb.num_columns):
            col, harr = db.column(i), hb.column(i)
            n = hb.num_rows
            assert col.null_count == harr.null_count
            if harr.null_count:
                assert harr.offset == 0
                assert np.array_equal(col.validity.cpu().numpy(), host_bits(harr.buffers()[0], n)), (k, i)
                assert col.validity.dtype.is_floating_point is False and str(col.validity.dtype) == "torch.bool"
            else:
                assert col.validity is None and col.validity_bits is None and harr.buffers()[0] is None
            if pa.types.is_boolean(harr.type):
                assert str(col.values.dtype) == "torch.bool"
                assert np.array_equal(col.values.cpu().numpy(), host_bits(harr.buffers()[1], n)), (k, i)
        db.release()
        count += 1
    assert count == len(want)
    assert rd.d2h_bytes() == 0
    rd.close()
    return count


@pytest.mark.parametrize("batch_size", BATCH_SIZES)
@pytest.mark.parametrize("name", FILES)
def test_parity_with_the_host_path(name, batch_size):
    n = assert_same_batches(A.data_path(name), batch_size)
    assert (n == 0) == (name == "TestOrcFile.emptyFile.orc")


def test_parity_without_read_ahead():
    assert assert_same_batches(A.data_path("nulls-at-end-snappy.orc"), 8192, prefetch=0) > 1


def test_parity_under_a_row_selection():
    """skips and selects inside a batch, across batches, and leaves a tail"""
    sel = [(300, True), (450, False), (1, True), (2100, False), (5000, True), (977, False), (40000, True), (20000, False)]
    for name, names in (("nulls-at-end-snappy.orc", None), ("lineitem_8k.zstd.orc", ["l_orderkey", "l_quantity", "l_comment", "l_shipdate"])):
        for prefetch in (0, 2):
            assert assert_same_batches(A.data_path(name), 1000, prefetch=prefetch, selection=sel, projection=names) > 2


def test_parity_under_a_predicate_and_a_row_filter():
    path = A.data_path("lineitem_8k.zstd.orc")
    assert assert_same_batches(path, 1000, predicate=P.gt("l_orderkey", V.Int64(1000))) >= 1
    for prune in (True, False):
        n = assert_same_batches(path, 1000, row_filter=P.gt("l_linenumber", V.Int32(3)), prune=prune)
        assert 1 <= n < 9  # (some rows go, some stay)
    # ... and the filter after a selection
    assert assert_same_batches(path, 1000, selection=[(100, True), (7000, False)], row_filter=P.gt("l_linenumber", V.Int32(3)), prune=False) >= 1


def test_tensors_are_the_decoders_buffers_and_nothing_crosses_the_link():
    import torch
    path = A.data_path("lineitem_8k.zstd.orc")
    rd = builder(path, 1000, True).build()
    seen = 0
    for db in rd:
        arr = db._array
        assert arr.device_type == 10 and arr.device_id == 0 and arr.sync_event
        assert arr.array.n_children == db.num_columns
        for i in range(db.num_columns):
            col = db.column(i)
            child = arr.array.children[i].contents
            assert child.length == db.num_rows
            if col.values is not None:
                assert col.values.is_cuda and col.values.data_ptr() == child.buffers[1]
                if pa.types.is_decimal(col.type):
                    assert tuple(col.values.shape) == (db.num_rows, 2) and col.values.dtype == torch.int64
                else:
                    assert tuple(col.values.shape) == (db.num_rows,)
            else:
                assert col.offsets.data_ptr() == child.buffers[1] and col.offsets.dtype == torch.int32 and col.offsets.numel() == db.num_rows + 1
                assert col.data.data_ptr() == child.buffers[2] and col.data.dtype == torch.uint8
                assert int(col.offsets[0]) == 0 and int(col.offsets[-1]) == col.data.numel()
            if col.null_count:
                assert col.validity_bits.data_ptr() == child.buffers[0]
            else:
                assert not child.buffers[0]
        seen += 1
    assert seen == 9 and rd.d2h_bytes() == 0
    rd.close()


def decode_stripes(name, batch_size):
    """The file's stripes without the reader: parsed by the tests' own ORC parser (orcfile), decoded through the stripe-level API.
    Yields (result, column names)."""
    f = orcfile.OrcFile(A.data_path(name))
    c = ctx()
    for s in f.stripes:
        cols, streams = [], []
        for cname, cid, typ in f.flat_columns():
            enc, dsz = s.encodings[cid] if cid < len(s.encodings) else (0, 0)
            cols.append({"column_id": cid, "orc_type": typ.kind, "encoding": enc, "dictionary_size": dsz, "precision": typ.precision,
                         "scale": typ.scale, "name": cname})
            streams += [(cid, k, v) for k, v in f.column_streams(s, cid).items()]
        staged = c.stage(s.number_of_rows, streams, cols, compression=f.compression_name, block_size=f.block_size, batch_size=batch_size,
                         writer_timezone=s.writer_timezone)
        res = c.decode([staged])[0]
        staged.free()
        assert res.status()[0] == 0
        yield res, [col["name"] for col in cols]


def expected_copy_bytes(name, batch_size, row_filter=None):
    """What a copy back of the file's stripes moves, derived without the reader: the stripes' column buffers' bytes as the
    stripe-level decode (and filter) laid them out."""
    total = 0
    for res, names in decode_stripes(name, batch_size):
        if row_filter is not None:
            ctx().result_filter(res, row_filter, names)
        total += res.buffer_bytes
        res.free()
    return total


def test_a_result_with_exports_out_is_not_rewritten():
    """decode into it again, select on it, filter it: refused while a device batch views it, and the batch stays what it was --
    also after the result is freed under it"""
    (res, names), = decode_stripes("lineitem_8k.zstd.orc", 1000)
    host = res.export_batch(2)
    db = res.export_batch_device(2)
    with pytest.raises(capi.OrcGpuError) as e:
        res.select([(10, True), (100, False)])
    assert e.value.code == INVALID
    with pytest.raises(capi.OrcGpuError) as e:
        ctx().result_filter(res, P.gt("l_linenumber", V.Int32(3)), names)
    assert e.value.code == INVALID
    x = db.column(0).values
    res.free()
    assert db.to_pyarrow().equals(host.rename_columns(db.schema.names))
    db.release()
    assert np.array_equal(x.cpu().numpy(), host.column(0).to_numpy())


@pytest.mark.parametrize("name", ["lineitem_8k.zstd.orc", "nulls-at-end-snappy.orc"])
def test_the_host_reader_counts_exactly_the_bytes_it_copies_back(name):
    """orcgpu_reader_d2h_bytes of a host reader equals the summed sizes of the stripes' column buffers -- whole arenas are copied,
    alignment gaps and all, so the figure is that of the buffers' layout, not of the Arrow buffers handed out, which bound it from
    below -- with and without read-ahead; under a row filter it is the kept rows' buffers alone."""
    want = expected_copy_bytes(name, 1000)
    for prefetch in (0, 2):
        rh = builder(A.data_path(name), 1000, False, prefetch).build()
        handed_out = 0
        for hb in rh:
            for arr in hb.columns:
                handed_out += sum(b.size for b in arr.buffers() if b is not None)
        got = rh.d2h_bytes()
        rh.close()
        assert got == want and 0 < handed_out <= got, (prefetch, got, want, handed_out)
    if name.startswith("lineitem"):
        pred = P.gt("l_linenumber", V.Int32(3))
        unfiltered, want = want, expected_copy_bytes(name, 1000, pred)
        assert 0 < want < unfiltered
        rh = builder(A.data_path(name), 1000, False, 2, row_filter=pred, prune=False).build()
        assert sum(b.num_rows for b in rh) > 0
        assert rh.d2h_bytes() == want
        rh.close()


def make_striped_file(n=20000):
    """Int64 + Utf8 rows written by this project's writer in many small stripes: (bytes, rows per stripe)"""
    rng = np.random.default_rng(5)
    x = rng.integers(-1 << 40, 1 << 40, n)
    s = ["row-%d-%s" % (i, "x" * int(k)) for i, k in enumerate(rng.integers(0, 9, n))]
    batch = pa.RecordBatch.from_pydict({"x": pa.array(x, pa.int64()), "s": pa.array(s)})
    out = io.BytesIO()
    w = ArrowWriterBuilder(out, batch.schema, ctx=ctx()).with_batch_size(1000).with_stripe_byte_size(2048).try_build()
    w.write(batch)
    w.close()
    rows = w.stripe_rows()
    w.free()
    return out.getvalue(), rows


@pytest.mark.parametrize("prefetch", (2, 0))
def test_tensors_outlive_their_batch_the_recycling_of_results_and_the_reader(prefetch):
    """The first stripe's tensors are kept, its batches dropped, the file read to its end -- every later stripe wants a result to
    decode into, and the first stripe's would be the spare one -- and the reader closed: the tensors still hold the first stripe."""
    import torch
    data, rows = make_striped_file()
    assert len(rows) >= 4 and sum(rows) == 20000
    rh = builder(data, 1000, False, prefetch).build()
    want, have = [], 0
    for hb in rh:
        if have < rows[0]:
            want.append(hb)
            have += hb.num_rows
    rh.close()
    assert have == rows[0]
    rd = builder(data, 1000, True, prefetch).build()
    kept, have, later = [], 0, 0
    for db in rd:
        if have < rows[0]:
            kept.append((db.column("x").values, db.column("s").offsets, db.column("s").data))
            have += db.num_rows
        else:
            later += db.num_rows
            assert int(db.column("x").values.numel()) == db.num_rows  # (consumed, then let go at once)
        db.release()
        del db
    gc.collect()
    assert later == 20000 - rows[0]
    rd.close()
    del rd
    gc.collect()
    torch.cuda.synchronize()
    assert len(kept) == len(want)
    for (x, off, dat), hb in zip(kept, want):
        assert np.array_equal(x.cpu().numpy(), hb.column("x").to_numpy())
        hs = hb.column("s")
        assert np.array_equal(off.cpu().numpy(), np.frombuffer(hs.buffers()[1], dtype=np.int32)[: len(hs) + 1])
        assert dat.cpu().numpy().tobytes() == hs.buffers()[2].to_pybytes()[: int(off[-1])]


def make_source(n=12000):
    """a file whose batches of 1000 rows all have the same nullability (a writer's schema is fixed): nulls in x and b, none in s and f"""
    rng = np.random.default_rng(9)
    x = pa.array(rng.integers(-1 << 30, 1 << 30, n), pa.int64(), mask=rng.random(n) < 0.15)
    s = pa.array(["k%03d" % k for k in rng.integers(0, 40, n)])
    f = pa.array(rng.standard_normal(n))
    b = pa.array(rng.random(n) < 0.5, pa.bool_(), mask=rng.random(n) < 0.1)
    out = io.BytesIO()
    orc.write_table(pa.table({"x": x, "s": s, "f": f, "b": b}), out, compression="zlib", stripe_size=64 << 10, batch_size=1000)
    return out.getvalue()


ROUND_TRIPS = {
    "plain": lambda b: b,
    "snappy": lambda b: b.with_compression("snappy"),
    "index_bloom": lambda b: b.with_row_index_stride(1000).with_bloom_filter_columns(["x"]),
    "dictionary": lambda b: b.with_dictionary_key_size_threshold(0.8),
}


@pytest.fixture(scope="module")
def source():
    return make_source()


@pytest.mark.parametrize("shared_context", (True, False))
@pytest.mark.parametrize("option", sorted(ROUND_TRIPS))
def test_round_trip_on_the_device_writes_the_host_paths_bytes(source, option, shared_context):
    """reader -> writer without the host in between: the file is the one of host reader -> host write.  shared_context: the writer
    on the reader's context (a reader that does not read ahead); else on one of its own beside a reader that does."""
    def write(device):
        prefetch = 0 if shared_context else 2
        r = builder(source, 1000, device, prefetch).build()
        out, w = io.BytesIO(), None
        for batch in r:
            if w is None:
                w = ROUND_TRIPS[option](ArrowWriterBuilder(out, batch.schema, ctx=ctx(0 if shared_context else 1)).with_batch_size(1000)
                                        .with_stripe_byte_size(16 << 10)).try_build()
            if device:
                w.write_device(batch)
                batch.release()
            else:
                w.write(batch)
        r.close()
        w.close()
        stripes = w.stats()["stripes"]
        w.free()
        return out.getvalue(), stripes
    want, stripes = write(False)
    assert stripes >= 2
    got, _ = write(True)
    assert got == want
    back = orc.ORCFile(io.BytesIO(got)).read()
    assert back.num_rows == 12000 and back.equals(orc.ORCFile(io.BytesIO(source)).read())


def test_write_device_refuses_a_context_that_reads_ahead():
    """(a file of many stripes: with two decoded ahead the reader's threads wait for the consumer, they have not ended)"""
    data, rows = make_striped_file()
    assert len(rows) >= 8
    r = builder(data, 1000, True, 2).build()
    batch = next(r)
    assert r.reads_ahead()
    w = ArrowWriterBuilder(io.BytesIO(), batch.schema, ctx=ctx()).try_build()
    with pytest.raises(ValueError):
        w.write_device(batch)
    w.free()
    batch.release()
    r.close()
    assert not r.reads_ahead()


@pytest.mark.parametrize("out_offset", (16, 5))
@pytest.mark.parametrize("n", UNPACK_SIZES)
def test_unpack_kernel_edges(n, out_offset):
    """n straddles the kernel's 16-byte store, a wavefront's 1024 output bytes and a workgroup's 4096; out_offset 16: an aligned
    output, 5: one whose first 11 bytes come in front of the first aligned store.  Nothing outside the two slices is touched."""
    import torch
    rng = np.random.default_rng(n * 31 + out_offset)
    nb = (n + 7) // 8
    bits = rng.integers(0, 256, nb, dtype=np.uint8)
    src = np.full(3 + nb + 64, 0xA5, dtype=np.uint8)
    src[3:3 + nb] = bits
    d_src = torch.from_numpy(src).cuda()
    d_out = torch.full((out_offset + n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    c = ctx()
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream or None
    c._check(c.L.orcgpu_unpack_bits(c.h, C.c_void_p(d_src.data_ptr() + 3), n, C.c_void_p(d_out.data_ptr() + out_offset), C.c_void_p(stream)))
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.array_equal(out[out_offset:out_offset + n], np.unpackbits(bits, bitorder="little")[:n])
    assert (out[:out_offset] == 0xA5).all() and (out[out_offset + n:] == 0xA5).all()
    assert np.array_equal(d_src.cpu().numpy(), src)


@pytest.fixture(scope="module")
def nested_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("device_output") / "nested.orc")
    orc.write_table(pa.table({"id": pa.array(range(3000), pa.int64()), "tags": pa.array([[i, i + 1] for i in range(3000)], pa.list_(pa.int32()))}), path)
    return path


def test_a_nested_column_is_refused_by_name_and_may_be_projected_away(nested_file):
    r = builder(nested_file, 1000, True).build()
    with pytest.raises(capi.OrcGpuError) as e:
        next(r)
    assert e.value.code == UNSUPPORTED and "'tags'" in str(e.value) and "List" in str(e.value)
    r.close()
    assert assert_same_batches(nested_file, 1000, projection=["id"]) == 3


def test_the_wrong_next_call_is_refused_and_the_reader_stays_usable(source):
    L = ctx().L
    want = builder(source, 1000, False).build()
    n_batches = len(list(want))
    want.close()
    a = (C.c_uint8 * 128)()
    s = (C.c_uint8 * 72)()
    rd = builder(source, 1000, True).build()
    assert L.orcgpu_reader_next_batch(rd._h, C.addressof(a), C.addressof(s)) == INVALID
    first = next(rd)
    assert L.orcgpu_reader_next_batch(rd._h, C.addressof(a), C.addressof(s)) == INVALID
    first.release()
    assert 1 + sum(1 for _ in rd) == n_batches
    rd.close()
    rh = builder(source, 1000, False).build()
    assert L.orcgpu_reader_next_batch_device(rh._h, C.addressof(a), C.addressof(s)) == INVALID
    assert sum(1 for _ in rh) == n_batches
    rh.close()
