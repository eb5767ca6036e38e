"""ArrowWriter's string dictionaries on the GPU (ArrowWriterBuilder.with_dictionary_key_size_threshold): every file is the model's
(tests/writer_dict_model.py, pinned by tests/test_writer_dict_model.py) byte for byte, is read back by pyarrow.orc and by
ArrowReaderBuilder (this project's DICTIONARY_V2 decode) equal to the input, and orcgpu_writer_dictionary_counts says which
path each (string column, stripe) took.  Shapes are chosen by where the table, the scans and the gather can go wrong."""
import ctypes as C
import io

import numpy as np
import pyarrow as pa
import pyarrow.orc as po
import pytest

import gpu_util as G
import oracle_lib as O
import writer_dict_model as DM
import writer_nested_model as NM
from orcfile import DATA, DICTIONARY_DATA, LENGTH, PRESENT, OrcFile
from orc_rust_amd import ArrowReaderBuilder, ArrowWriterBuilder, capi
from orc_rust_amd.capi import OrcGpuError
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
from test_gpu_writer import _ArrowArray, _lineitem
from test_gpu_writer_compression import check_chunked
from test_gpu_writer_index import _read, same_values

pytestmark = pytest.mark.gpu

UNEXPECTED, INVALID_ARGUMENT = 10, 101  # include/orcgpu.h


def gpu_write(batches, t=None, schema=None, batch_size=1024, sbs=64 << 20, flush_after=(), comp=None, block=4096, stride=0):
    out = io.BytesIO()
    b = ArrowWriterBuilder(out, schema or batches[0].schema, ctx=G.ctx()).with_batch_size(batch_size).with_stripe_byte_size(sbs)
    if t is not None:
        b = b.with_dictionary_key_size_threshold(t)
    if comp:
        b = b.with_compression(comp, block)
    if stride:
        b = b.with_row_index_stride(stride)
    w = b.try_build()
    for i, x in enumerate(batches):
        w.write(x)
        if i in flush_after:
            w.flush_stripe()
    w.close()
    rows, stats, counts = w.stripe_rows(), w.stats(), w.dictionary_counts()
    w.free()
    return out.getvalue(), rows, stats, counts


def readers(data, batches, schema=None):
    want = NM.read_types(pa.Table.from_batches(batches, schema=schema))
    assert po.ORCFile(io.BytesIO(data)).read().equals(want), "pyarrow.orc read back something else"
    mine = list(ArrowReaderBuilder.try_new(data, ctx=G.ctx()).build())
    assert sum(b.num_rows for b in mine) == want.num_rows
    if want.num_rows:
        for i, f in enumerate(want.schema):
            got = pa.concat_arrays([b.column(i) for b in mine])
            if pa.types.is_nested(f.type):
                assert got.to_pylist() == want.column(i).to_pylist(), "ArrowReaderBuilder read back something else in %s" % f.name
            else:
                assert got.equals(want.column(i).combine_chunks()), "ArrowReaderBuilder read back something else in %s" % f.name


def check(batches, t, schema=None, batch_size=1024, sbs=64 << 20, flush_after=(), stride=0):
    O.lib()
    info = {}
    want, want_rows = DM.write_model(batches, schema=schema, batch_size=batch_size, stripe_byte_size=sbs, flush_after=flush_after, threshold=t,
                                     row_index_stride=stride, info=info)
    got, rows, stats, counts = gpu_write(batches, t, schema, batch_size, sbs, flush_after, stride=stride)
    assert rows == want_rows, (rows, want_rows)
    assert counts == {"dictionary": info["dictionary"], "direct": info["direct"]}, (counts, info)
    assert got == want, "file bytes differ from the model's (%d vs %d bytes)" % (len(got), len(want))
    readers(got, batches, schema)
    return info, stats


def one(values, t=pa.string()):
    return pa.RecordBatch.from_arrays([pa.array(values, type=t)], names=["s"])


def cycle(n, d, fmt="k%d"):
    return [fmt % (i % d) for i in range(n)]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_few_rows(n):
    info, _ = check([one(cycle(n, 5))], 1.0)
    assert info["decisions"] == [{1: min(n, 5)}]


def test_all_rows_equal_and_all_distinct():
    info, _ = check([one(["same value"] * 3000)], 0.01)
    assert info["decisions"] == [{1: 1}]
    distinct = ["s%d" % i for i in range(3000)]
    info, _ = check([one(distinct)], 1.0)
    assert info["decisions"] == [{1: 3000}]
    info, _ = check([one(distinct)], 0.999)
    assert info["decisions"] == [{1: None}]


def test_rule_boundary():
    assert check([one(["a", "b", "c", "d", "e"] * 2)], 0.5)[0]["decisions"] == [{1: 5}]
    assert check([one(["a", "b", "c", "d", "e", "f", "a", "b", "c", "d"])], 0.5)[0]["decisions"] == [{1: None}]


def test_empty_strings_and_nulls():
    assert check([one([""] * 100)], 0.5)[0]["decisions"] == [{1: 1}]
    assert check([one(["", None, "", None, "x", ""] * 30)], 0.5)[0]["decisions"] == [{1: 2}]
    assert check([one(["", "a", "", "", "bc", ""] * 30)], 0.5)[0]["decisions"] == [{1: 3}]
    schema = pa.schema([("s", pa.string())])
    nulls = pa.RecordBatch.from_arrays([pa.array([None] * 200, type=pa.string())], schema=schema)
    info, _ = check([nulls, nulls.slice(0, 0)], 1.0, schema=schema, flush_after=(0, 1))  # ... and a stripe of 0 rows
    assert info["decisions"] == [{1: None}, {1: None}]


def test_value_lengths():
    """0 .. 300 bytes: pairs that differ in their last byte alone, a value that is a prefix of another, the 16-byte steps' and the
    wavefront's limits"""
    rng = np.random.default_rng(1)
    vals = []
    for n in list(range(0, 40)) + [63, 64, 65, 127, 128, 129, 255, 256, 257, 299, 300]:
        base = bytes(rng.integers(97, 123, n, dtype=np.uint8)).decode()
        vals.append(base)
        if n:
            vals.append(base[:-1] + ("A" if base[-1] != "A" else "B"))  # the last byte alone
            vals.append(base[:-1])                                      # a prefix
    d = len(set(vals))
    rows = [vals[i] for i in rng.integers(0, len(vals), 4000)] + vals
    info, _ = check([one(rows)], 1.0)
    assert info["decisions"] == [{1: d}]


@pytest.mark.parametrize("d", [255, 256, 257, 512, 513])
def test_dictionary_sizes(d):
    """the entries' LENGTH runs (512 values at most), ids across a byte's range"""
    assert check([one(cycle(3 * d + 7, d, "%d"))], 1.0)[0]["decisions"] == [{1: d}]


def test_ids_past_two_bytes():
    d = 70000
    rng = np.random.default_rng(2)
    rows = ["%x" % i for i in range(d)] + ["%x" % i for i in rng.integers(0, d, 30000)]
    got, rows_, _, counts = gpu_write([one(rows)], 1.0)
    f = OrcFile(got)
    assert counts == {"dictionary": 1, "direct": 0} and f.stripes[0].encodings[1] == (3, d)
    O.lib()
    st, ids = O.int_rle(bytes(f.stripes[0].streams[(1, DATA)]), len(rows), signed=False)
    assert st == 0 and ids[:d].tolist() == list(range(d)) and ids.max() == d - 1
    want, _ = DM.write_model([one(rows)], threshold=1.0)
    assert got == want
    readers(got, [one(rows)])


def test_sliced_large_and_several_writes():
    rng = np.random.default_rng(3)
    v = ["w%d" % x * (x % 4) for x in rng.integers(0, 40, 5000)]
    b = pa.RecordBatch.from_arrays([pa.array(v, mask=rng.random(5000) < 0.2), pa.array(v, type=pa.large_string())], names=["s", "ls"])
    info, _ = check([b.slice(13, 2000), b.slice(1001, 1777), b.slice(4999, 1)], 0.5, batch_size=100)  # one stripe, three writes
    assert len(info["decisions"]) == 1 and all(x is not None for x in info["decisions"][0].values())


def test_one_write_cut_into_stripes():
    """the second stripe's ids start at 0 again"""
    b = one(cycle(6000, 11, "value-%d"))
    info, _ = check([b], 0.5, batch_size=500, sbs=20000)
    assert len(info["decisions"]) >= 2 and all(x == {1: 11} for x in info["decisions"])


def test_dictionary_then_direct():
    """high-cardinality rows after low-cardinality ones: the column changes its encoding from one stripe to the next"""
    low, high = cycle(4000, 3, "low%d"), ["high%d" % i for i in range(4000)]
    info, _ = check([one(low), one(high)], 0.5, flush_after=(0,))
    assert info["decisions"] == [{1: 3}, {1: None}]
    f = OrcFile(gpu_write([one(low), one(high)], 0.5, flush_after=(0,))[0])
    assert [s.encodings[1] for s in f.stripes] == [(3, 3), (2, 0)]


def test_sticky_present():
    """PRESENT begins in a later stripe (back-filled within it) and stays"""
    plain, holes = one(cycle(900, 4)), one([None if i % 5 == 0 else "k%d" % (i % 4) for i in range(900)])
    info, _ = check([plain, plain, holes, plain], 0.5, flush_after=(0, 2))
    assert info["decisions"] == [{1: 4}] * 3


def test_columns_beside_each_other():
    rng = np.random.default_rng(4)
    n = 3000
    b = pa.RecordBatch.from_arrays(
        [pa.array(cycle(n, 6), mask=rng.random(n) < 0.1), pa.array(rng.integers(0, 99, n)), pa.array(rng.integers(0, 9, n).astype(np.int32)),
         pa.array(cycle(n, 9, "second-%d")), pa.array([b"bin%d" % (i % 3) for i in range(n)], type=pa.binary())], names=["a", "i", "j", "b", "bin"])
    info, _ = check([b], 0.8)
    assert info["decisions"] == [{1: 6, 4: 9}]
    s = OrcFile(gpu_write([b], 0.8)[0]).stripes[0]
    assert [(c, k) for k, c, _ in s.stream_list] == [(1, DATA), (1, LENGTH), (1, DICTIONARY_DATA), (1, PRESENT), (2, DATA), (3, DATA), (4, DATA),
                                                     (4, LENGTH), (4, DICTIONARY_DATA), (5, DATA), (5, LENGTH)]
    assert s.encodings == [(0, 0), (3, 6), (2, 0), (2, 0), (3, 9), (2, 0)]


def test_hash_bits_switch(monkeypatch):
    """ORCGPU_DICT_HASH_BITS=2: four home slots for 300 strings, so long probe sequences -- and not a byte of difference"""
    rng = np.random.default_rng(5)
    b = one(["entry-%d" % x for x in rng.integers(0, 300, 5000)])
    want = gpu_write([b], 0.5)[0]
    monkeypatch.setenv("ORCGPU_DICT_HASH_BITS", "2")
    got, _, _, counts = gpu_write([b], 0.5)
    monkeypatch.delenv("ORCGPU_DICT_HASH_BITS")
    assert got == want and counts == {"dictionary": 1, "direct": 0}
    O.lib()
    assert got == DM.write_model([b], threshold=0.5)[0]


def test_same_bytes_every_time():
    rng = np.random.default_rng(6)
    b = one(["r%d" % x for x in rng.integers(0, 2000, 50000)])
    files = [gpu_write([b], 0.5)[0] for _ in range(3)]
    assert files[0] == files[1] == files[2]
    assert OrcFile(files[0]).stripes[0].encodings[1][0] == 3


@pytest.mark.parametrize("codec", ["snappy", "lz4"])
def test_compressed(codec):
    rng = np.random.default_rng(7)
    n = 6000
    b = pa.RecordBatch.from_arrays([pa.array(cycle(n, 12, "compressible-%d"), mask=rng.random(n) < 0.1), pa.array(rng.integers(0, 9, n))], names=["s", "i"])
    plain = gpu_write([b], 0.5, batch_size=500, sbs=30000)[0]
    got, _, _, counts = gpu_write([b], 0.5, batch_size=500, sbs=30000, comp=codec, block=1024)
    assert counts["dictionary"] == len(OrcFile(plain).stripes) > 1 and counts["direct"] == 0
    check_chunked(got, plain, codec, 1024)
    readers(got, [b])


def test_row_index():
    rng = np.random.default_rng(8)
    n, S = 10000, 1000
    keys = np.sort(rng.integers(0, 40, n))
    b = pa.RecordBatch.from_arrays([pa.array(["key%02d" % k for k in keys], mask=rng.random(n) < 0.1), pa.array(np.arange(n, dtype=np.int64))], names=["s", "i"])
    info, _ = check([b], 0.5, stride=S)
    assert info["decisions"] == [{1: 40}]
    data = gpu_write([b], 0.5, stride=S)[0]
    whole, _ = _read(data)
    assert whole.num_rows == n
    # a row selection and a predicate that prune row groups: the rows of the unpruned read, found through the positions
    for g in (0, 3, 9):
        sel = ([(g * S, True)] if g else []) + [(S, False)] + ([(n - (g + 1) * S, True)] if g < 9 else [])
        got, groups = _read(data, selection=sel)
        assert groups == (1, 10) and same_values(got, whole.slice(g * S, S)), g
    got, groups = _read(data, predicate=P.gte("i", V.Int64(7500)))
    assert groups == (3, 10) and same_values(got, whole.slice(7000, 3000))
    got, groups = _read(data, predicate=P.lt("s", V.Utf8("key05")))
    assert 0 < groups[0] < 10 and same_values(got, whole.slice(0, groups[0] * S))
    # ... compressed as well: the positions go through the chunk map
    comp = gpu_write([b], 0.5, stride=S, comp="snappy", block=1024)[0]
    got, groups = _read(comp, predicate=P.gte("i", V.Int64(7500)))
    assert groups == (3, 10) and same_values(got, whole.slice(7000, 3000))


def test_nested_strings():
    rng = np.random.default_rng(9)
    n = 3000

    def strs(k, d=7):
        return pa.array(["item%d" % x for x in rng.integers(0, d, k)], mask=rng.random(k) < 0.1)
    lst = NM.list_array(n, rng, strs, nulls=0.2)
    st = pa.StructArray.from_arrays([strs(n, 4)], names=["s"], mask=pa.array(rng.random(n) < 0.2))
    b = pa.RecordBatch.from_arrays([lst, st], names=["l", "st"])
    info, stats = check([b], 0.8, batch_size=700)
    assert info["decisions"] == [{2: 7, 4: 4}]
    assert stats["nested_gathers"] > 0


def test_device_batch_from_the_reader():
    """a string batch the GPU decoder produced, written from its device buffers (ORCGPU_ENC_ON_DEVICE): the bytes of the host's"""
    from orc_rust_amd import gen
    rng = np.random.default_rng(10)
    n = 20000
    present = (rng.random(n) > 0.15).astype(np.uint8)
    k = int(present.sum())
    words = [b"dev%d" % x for x in rng.integers(0, 25, k)]
    cols = [{"column_id": 1, "orc_type": 7, "encoding": 2}]
    streams = [(1, 0, gen.boolean(present)), (1, 1, b"".join(words)), (1, 2, gen.rle2(np.array([len(x) for x in words], dtype=np.int64), signed=False))]
    res = G.gpu_decode(n, cols, streams, batch_size=8192)
    assert res.status()[0] == 0
    v = res.view(1, 0)  # the second batch
    host = res.batch(1, 0)
    m = v.length
    valid = np.unpackbits(np.frombuffer(host["validity"], dtype=np.uint8), bitorder="little")[:m].astype(bool)
    offs, vals = host["offsets"], bytes(host["values"])
    hb = one([vals[offs[i]:offs[i + 1]].decode() if valid[i] else None for i in range(m)])
    want, _, _, counts = gpu_write([hb], 0.5, batch_size=1000)
    assert counts == {"dictionary": 1, "direct": 0}
    child = _ArrowArray()
    cbufs = (C.c_void_p * 3)(v.validity, v.offsets, v.values)
    child.length, child.null_count, child.offset, child.n_buffers, child.n_children, child.buffers = m, v.null_count, 0, 3, 0, cbufs
    root = _ArrowArray()
    rbufs = (C.c_void_p * 1)(None)
    kids = (C.POINTER(_ArrowArray) * 1)(C.pointer(child))
    root.length, root.null_count, root.offset, root.n_buffers, root.n_children, root.buffers, root.children = m, 0, 0, 1, 1, rbufs, kids
    out = io.BytesIO()
    w = ArrowWriterBuilder(out, hb.schema, ctx=G.ctx()).with_batch_size(1000).with_dictionary_key_size_threshold(0.5).try_build()
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
    O.lib()
    assert want == DM.write_model([hb], batch_size=1000, threshold=0.5)[0]
    readers(want, [hb])


def _waits_per_stripe(ncols, t):
    b = pa.RecordBatch.from_arrays([pa.array(cycle(5000, 5 + c, "c%d")) for c in range(ncols)], names=["s%d" % c for c in range(ncols)])
    b0 = ArrowWriterBuilder(io.BytesIO(), b.schema, ctx=G.ctx())
    w = (b0.with_dictionary_key_size_threshold(t) if t is not None else b0).try_build()
    w.write(b)
    w.flush_stripe()  # (the buffers grow in the first stripe)
    s0 = w.stats()
    for _ in range(3):
        w.write(b)
        w.flush_stripe()
    s1, counts = w.stats(), w.dictionary_counts()
    w.close()
    w.free()
    return (s1["stripe_round_trips"] - s0["stripe_round_trips"]) // 3, (s1["round_trips"] - s0["round_trips"]) // 3, counts


def test_host_waits_do_not_grow_with_the_columns():
    one_col, six = _waits_per_stripe(1, 0.5), _waits_per_stripe(6, 0.5)
    assert one_col[:2] == six[:2]
    assert one_col[2] == {"dictionary": 4, "direct": 0} and six[2] == {"dictionary": 24, "direct": 0}
    plain = _waits_per_stripe(6, None)
    assert six[0] == plain[0] + 1  # one wait more a stripe: the columns' (n, d) come back together


def test_threshold_zero_is_the_default():
    never, zero = _waits_per_stripe(3, None), _waits_per_stripe(3, 0.0)
    assert never == zero and zero[2] == {"dictionary": 0, "direct": 12}
    rng = np.random.default_rng(11)
    b = pa.RecordBatch.from_arrays([pa.array(cycle(4000, 5)), pa.array(rng.integers(0, 9, 4000))], names=["s", "i"])
    a, rows_a, stats_a, _ = gpu_write([b], None, batch_size=300, sbs=4096)
    z, rows_z, stats_z, _ = gpu_write([b], 0.0, batch_size=300, sbs=4096)
    assert a == z and rows_a == rows_z and stats_a == stats_z


def test_setter_errors():
    b = one(["a", "b"])
    w = ArrowWriterBuilder(io.BytesIO(), b.schema, ctx=G.ctx()).try_build()
    L = G.ctx().L
    for bad in (float("nan"), -0.1, 1.5):
        assert L.orcgpu_writer_set_dictionary(w._h, bad) == INVALID_ARGUMENT
    assert L.orcgpu_writer_set_dictionary(w._h, 1.0) == 0
    w.write(b)
    assert L.orcgpu_writer_set_dictionary(w._h, 0.5) == INVALID_ARGUMENT  # as set_compression after a write
    assert L.orcgpu_writer_set_compression(w._h, 2, 0) == INVALID_ARGUMENT
    w.close()
    assert w.dictionary_counts() == {"dictionary": 1, "direct": 0}
    w.free()


def test_lineitem():
    """300 000 lineitem-shaped rows, t = 0.8: the low-cardinality string columns go dictionary, the comment-like one direct, and
    the file is smaller than the same table's without a threshold (3 to 25-byte values over fewer than 10 distinct strings: a byte
    or less per row of ids against the values' bytes and a length each)"""
    rng = np.random.default_rng(12)
    n = 300_000
    b = _lineitem(n, rng)
    batches = [b.slice(i, 100_000) for i in range(0, n, 100_000)]
    plain, rows0, _, c0 = gpu_write(batches)
    got, rows, _, counts = gpu_write(batches, 0.8)
    assert rows == rows0 and sum(rows) == n
    names = b.schema.names
    low = [names.index(x) + 1 for x in ("l_returnflag", "l_linestatus", "l_shipinstruct", "l_shipmode")]
    comment = names.index("l_comment") + 1
    for s in OrcFile(got).stripes:
        assert [s.encodings[c] for c in low] == [(3, 3), (3, 2), (3, 4), (3, 7)]
        assert s.encodings[comment] == (2, 0)
    assert counts == {"dictionary": 4 * len(rows), "direct": len(rows)} and c0 == {"dictionary": 0, "direct": 5 * len(rows)}
    assert len(got) < len(plain)
    print("lineitem %d rows: %d bytes with dictionaries, %d without (%.4f)" % (n, len(got), len(plain), len(got) / len(plain)))
    assert po.ORCFile(io.BytesIO(got)).read().equals(pa.Table.from_batches(batches))
    mine = pa.Table.from_batches(list(ArrowReaderBuilder.try_new(got, ctx=G.ctx()).build()))
    assert same_values(mine, pa.Table.from_batches(batches))
    # the bytes against the model on a share small enough for it
    check([b.slice(0, 40_000)], 0.8, sbs=1 << 20)
