"""The Python model of the writer's string dictionaries (tests/writer_dict_model.py) against two independent readers -- pyarrow.orc
(Apache ORC C++) and the oracle -- and the rule's boundary.  CPU only: this pins the model that tests/test_gpu_writer_dictionary.py
holds the device writer to byte for byte."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.orc as po
import pytest

import oracle_lib as O
import oracle_nested as ON
import writer_dict_model as DM
import writer_model as WM
import writer_nested_model as NM
from orcfile import DATA, DICTIONARY_DATA, LENGTH, PRESENT, OrcFile


def _strings(n, d, rng, nulls=0.0, t=pa.string()):
    v = ["v%d" % x * (1 + x % 3) for x in rng.integers(0, d, n)]
    return pa.array(v, type=t, mask=(rng.random(n) < nulls) if nulls else None)


def _check_readers(data, batches):
    want = NM.read_types(pa.Table.from_batches(batches))
    assert po.ORCFile(io.BytesIO(data)).read().equals(want)
    f = OrcFile(data)
    at = 0
    for s in f.stripes:  # the oracle, stripe by stripe, the flat string columns
        for name, cid, t in f.root_columns():
            if t.kind != 7:
                continue
            got = ON.Leaf(f, s, cid).next_batch(s.number_of_rows, None)
            assert got.equals(want.column(name).combine_chunks().slice(at, s.number_of_rows)), (name, at)
        at += s.number_of_rows


def _encodings(data):
    return [s.encodings for s in OrcFile(data).stripes]


@pytest.mark.parametrize("nulls", [0.0, 0.3])
@pytest.mark.parametrize("t", [0.5, 1.0])
def test_round_trip(nulls, t):
    O.lib()
    rng = np.random.default_rng(int(t * 10) + (nulls > 0))
    n = 3000
    b = pa.RecordBatch.from_arrays([_strings(n, 9, rng, nulls), pa.array(rng.integers(0, 99, n)), _strings(n, 5000, rng, nulls, pa.large_string()),
                                    pa.array([b"x%d" % (i % 3) for i in range(n)], type=pa.binary())], names=["lo", "i", "hi", "bin"])
    info = {}
    data, rows = DM.write_model([b], batch_size=100, stripe_byte_size=8192, threshold=t, info=info)
    assert len(rows) > 1 and info["dictionary"] >= len(rows)
    plain, rows0 = WM.write_model([b], batch_size=100, stripe_byte_size=8192)
    assert rows == rows0  # the cut does not move
    _check_readers(data, [b])
    for enc in _encodings(data):
        assert enc[1][0] == 3 and enc[2] == (2, 0) and enc[4] == (2, 0)  # the Binary column stays DIRECT_V2
        assert (enc[3][0] == 3) == (t == 1.0)
    s = OrcFile(data).stripes[0]
    assert [k for k, c, _ in s.stream_list if c == 1] == ([DATA, LENGTH, DICTIONARY_DATA] + ([PRESENT] if nulls else []))


def test_threshold_zero_is_writer_model():
    O.lib()
    rng = np.random.default_rng(5)
    b = pa.RecordBatch.from_arrays([_strings(2000, 4, rng, 0.1), pa.array(rng.integers(0, 9, 2000))], names=["s", "i"])
    want = WM.write_model([b], batch_size=64, stripe_byte_size=2048)
    assert DM.write_model([b], batch_size=64, stripe_byte_size=2048) == want
    info = {}
    assert DM.write_model([b], batch_size=64, stripe_byte_size=2048, threshold=0.0, info=info) == want
    assert info["dictionary"] == 0 and info["direct"] == len(want[1])


def _one(values, t, **kw):
    b = pa.RecordBatch.from_arrays([pa.array(values, type=pa.string())], names=["s"])
    info = {}
    data, _ = DM.write_model([b], threshold=t, info=info, **kw)
    return data, b, info


def test_rule_boundary():
    O.lib()
    five, six = ["a", "b", "c", "d", "e"] * 2, ["a", "b", "c", "d", "e", "f", "a", "b", "c", "d"]
    data, b, info = _one(five, 0.5)  # n = 10, d = 5
    assert _encodings(data) == [[(0, 0), (3, 5)]] and info["decisions"] == [{1: 5}]
    _check_readers(data, [b])
    data, b, info = _one(six, 0.5)  # n = 10, d = 6
    assert _encodings(data) == [[(0, 0), (2, 0)]] and info["decisions"] == [{1: None}]
    assert data == WM.write_model([b])[0]
    distinct = ["s%d" % i for i in range(100)]
    data, b, _ = _one(distinct, 1.0)
    assert _encodings(data) == [[(0, 0), (3, 100)]]
    _check_readers(data, [b])
    data, b, _ = _one(distinct, 0.999)
    assert data == WM.write_model([b])[0]
    assert DM.is_dictionary(10, 5, 0.5) and not DM.is_dictionary(10, 6, 0.5) and not DM.is_dictionary(0, 0, 1.0) and not DM.is_dictionary(5, 1, 0.0)


def test_first_occurrence_order_and_ids_restart():
    O.lib()
    v = ["z", "a", "z", "", "m", "a", ""] * 40
    b = pa.RecordBatch.from_arrays([pa.array(v)], names=["s"])
    data, rows = DM.write_model([b, b], threshold=1.0, flush_after=(0,))
    assert rows == [280, 280]
    f = OrcFile(data)
    for s in f.stripes:
        assert bytes(s.streams[(1, DICTIONARY_DATA)]) == b"zam" and s.encodings[1] == (3, 4)
        st, lens = O.int_rle(bytes(s.streams[(1, LENGTH)]), 4, signed=False)
        assert st == 0 and list(lens) == [1, 1, 0, 1]
        st, ids = O.int_rle(bytes(s.streams[(1, DATA)]), 280, signed=False)
        assert st == 0 and list(ids) == [0, 1, 0, 2, 3, 1, 2] * 40
    _check_readers(data, [b, b])


def test_all_null_and_zero_row_stripe_are_direct():
    O.lib()
    schema = pa.schema([("s", pa.string())])
    nulls = pa.RecordBatch.from_arrays([pa.array([None] * 50, type=pa.string())], schema=schema)
    info = {}
    empty = nulls.slice(0, 0)
    data, rows = DM.write_model([nulls, empty], schema=schema, threshold=1.0, flush_after=(0, 1), info=info)
    assert rows == [50, 0] and info == {"dictionary": 0, "direct": 2, "decisions": [{1: None}, {1: None}]}
    assert data == WM.write_model([nulls, empty], schema=schema, flush_after=(0, 1))[0]
    assert po.ORCFile(io.BytesIO(data)).read().equals(pa.Table.from_batches([nulls]))


def test_nested_strings():
    O.lib()
    rng = np.random.default_rng(3)
    n = 500
    lst = NM.list_array(n, rng, lambda k: _strings(k, 6, rng, 0.1), nulls=0.2)
    st = pa.StructArray.from_arrays([_strings(n, 3, rng, 0.1)], names=["s"], mask=pa.array(rng.random(n) < 0.2))
    b = pa.RecordBatch.from_arrays([lst, st], names=["l", "st"])
    info = {}
    data, rows = DM.write_model([b], threshold=0.8, info=info)
    assert info["decisions"] == [{2: 6, 4: 3}]
    assert po.ORCFile(io.BytesIO(data)).read().equals(pa.Table.from_batches([b]))


def test_row_index_positions_of_a_dictionary_column():
    O.lib()
    import index_model as IM
    rng = np.random.default_rng(4)
    n = 5000
    b = pa.RecordBatch.from_arrays([_strings(n, 7, rng, 0.2), pa.array(rng.integers(0, 50, n))], names=["s", "i"])
    data, rows = DM.write_model([b], threshold=0.8, row_index_stride=1000)
    f = OrcFile(data)
    assert f.row_index_stride == 1000 and f.stripes[0].encodings[1] == (3, 7)
    entries = IM.row_index_entries(f, f.stripes[0], 1)
    assert len(entries) == 5 and all(len(pos) == 5 for pos, _ in entries)  # PRESENT: 3, the ids: 2
    assert [st["n"] for _, st in entries] == [int(np.asarray(b.column(0).slice(g * 1000, 1000).is_valid()).sum()) for g in range(5)]
    got = po.ORCFile(io.BytesIO(data))
    assert got.read().equals(pa.Table.from_batches([b])) and got.nstripe_statistics == 1
