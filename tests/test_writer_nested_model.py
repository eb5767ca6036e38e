"""The nested writer's model (tests/writer_nested_model.py) judged without a GPU: its files are read by pyarrow.orc (Apache ORC
C++) equal to the input tables, and every stream of every column, decoded by the CPU oracle and reassembled by
tests/oracle_nested.py, gives the input back."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.orc as po
import pytest

import oracle_lib as O
import oracle_nested as N
import writer_model as WM
import writer_nested_model as NM
import writer_types_model as TM
from orcfile import OrcFile
from writer_nested_model import ints, list_array, map_array, raw_list, strings


def check_model(batches, **kw):
    O.lib()
    data, rows = NM.write_model(batches, **kw)
    want = NM.read_types(pa.Table.from_batches(batches))
    got = po.ORCFile(io.BytesIO(data)).read()
    assert got.equals(want), "pyarrow.orc read the model's file as something else"
    f = OrcFile(data)
    assert sum(rows) == want.num_rows
    for name, cid, typ in f.root_columns():
        if typ.kind in (N.STRUCT, N.LIST, N.MAP):
            chunks = N.read_column(f, cid, 1000)
            mine = pa.chunked_array(chunks).to_pylist() if chunks else []
            assert mine == want.column(name).to_pylist(), "the oracle decodes column %s to something else" % name
    return data, rows


def depth3(n, rng, nulls=0.1):
    def structs(m):
        a = list_array(m, rng, ints(rng, np.int32, nulls), nulls=nulls)
        s = strings(rng, nulls)(m)
        return pa.StructArray.from_arrays([a, s], names=["a", "s"], mask=pa.array(rng.random(m) < nulls) if nulls else None)
    return list_array(n, rng, structs, nulls=nulls)


def test_depth_three_list_of_struct_of_list():
    rng = np.random.default_rng(3)
    b = pa.RecordBatch.from_arrays([depth3(200, rng), pa.array(np.arange(200, dtype=np.int64))], names=["l", "i"])
    assert str(b.schema.field("l").type) == "list<item: struct<a: list<item: int32>, s: string>>"
    check_model([b, b.slice(7, 90)], batch_size=16)


def test_map_large_list_struct_of_struct_and_decimal_under_struct():
    rng = np.random.default_rng(5)
    n = 150
    keys = list_array(n, rng, strings(rng), nulls=0.1)
    vals = pa.array(rng.random(len(keys.values)), mask=rng.random(len(keys.values)) < 0.2)
    m = map_array(keys, vals)
    ll = list_array(n, rng, ints(rng, np.int64, 0.1), nulls=0.1, large=True)
    inner = pa.StructArray.from_arrays([pa.array(rng.integers(0, 9, n).astype(np.int16)), strings(rng, 0.1)(n)], names=["x", "y"],
                                       mask=pa.array(rng.random(n) < 0.2))
    dec = TM.dec_array([int(v) for v in rng.integers(-10 ** 9, 10 ** 9, n)], 20, 3, rng.random(n) < 0.1)
    outer = pa.StructArray.from_arrays([inner, dec, pa.array(rng.random(n) < 0.5)], names=["in", "d", "b"], mask=pa.array(rng.random(n) < 0.2))
    b = pa.RecordBatch.from_arrays([m, ll, outer], names=["m", "ll", "ss"])
    assert b.schema.field("m").type == pa.map_(pa.string(), pa.float64()) and b.schema.field("ll").type == pa.large_list(pa.int64())
    data, _ = check_model([b, b.slice(3, 100), b.slice(149, 1)], batch_size=32)
    f = OrcFile(data)
    assert [t.kind for t in f.types] == [12, 11, 7, 6, 10, 4, 12, 12, 2, 7, 14, 0]
    assert list(f.types[6].subtypes) == [7, 10, 11] and list(f.types[7].subtypes) == [8, 9] and list(f.types[1].subtypes) == [2, 3]


def test_null_lists_that_own_ranges_and_the_cut_between_long_lists():
    rng = np.random.default_rng(11)
    a = list_array(300, rng, ints(rng, np.int32), nulls=0.3, max_len=40)
    b = pa.RecordBatch.from_arrays([a], names=["l"])
    for bs in (1, 7):
        data, rows = check_model([b, b], batch_size=bs, stripe_byte_size=600, flush_after=(0,))
        assert len(rows) > 4
    # a zero-row stripe, and PRESENT appearing from the second batch on (back-filled)
    plain = pa.RecordBatch.from_arrays([list_array(50, rng, ints(rng, np.int32))], names=["l"])
    nulls = pa.RecordBatch.from_arrays([list_array(50, rng, ints(rng, np.int32, 0.3), nulls=0.3)], names=["l"])
    data, rows = check_model([plain, nulls], flush_after=(1,))
    m = NM.WriterModel(plain.schema)
    m.write(plain)
    m.flush_stripe()
    m.flush_stripe()
    assert m.stripe_rows() == [50, 0]


def test_flat_schemas_are_the_flat_models_files():
    rng = np.random.default_rng(2)
    t = TM.mixed_table(300, rng)
    bs = [t, t.slice(5, 100)]
    assert NM.write_model(bs, batch_size=64, stripe_byte_size=2000) == TM.write_model(bs, batch_size=64, stripe_byte_size=2000)
    b = pa.RecordBatch.from_arrays([pa.array(np.arange(100, dtype=np.int32)), pa.array(["a"] * 100)], names=["i", "s"])
    assert NM.write_model([b]) == WM.write_model([b])


@pytest.mark.parametrize("t", [pa.list_(pa.int32(), 3), pa.list_view(pa.int32()), pa.dense_union([pa.field("a", pa.int32())]),
                               pa.dictionary(pa.int32(), pa.string()), pa.run_end_encoded(pa.int32(), pa.int64()), pa.list_(pa.decimal128(10, 2)),
                               pa.map_(pa.string(), pa.decimal128(10, 2)), pa.struct([("s", pa.list_(pa.date32()))]), pa.decimal256(40, 2)])
def test_unsupported_shapes_are_rejected_with_their_path(t):
    with pytest.raises(NotImplementedError) as e:
        NM.WriterModel(pa.schema([("top", pa.struct([("x", t)]))]))
    assert "top.x" in str(e.value)


def test_bad_offsets_reject_the_batch_and_nothing_else():
    rng = np.random.default_rng(9)
    good = pa.RecordBatch.from_arrays([list_array(20, rng, ints(rng, np.int32))], names=["l"])
    child = pa.array(np.arange(10, dtype=np.int32))
    for offs in ([0, 4, 2, 6], [0, 100, 6, 9]):
        bad = pa.RecordBatch.from_arrays([raw_list(offs, child)], names=["l"])
        assert NM.write_model([good, bad, good]) == NM.write_model([good, good])
