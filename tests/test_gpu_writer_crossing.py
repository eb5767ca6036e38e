"""ArrowWriter's features crossed in one file each: every flat type beside the others with nulls, a row index, a dictionary, two
stripes and compression; and a Struct of a List and a Map beside a plain column, compressed.  The other test_gpu_writer*.py each
take one feature; the description of a column's streams (orcgpu_writer_host.inc: wr_streams) is where they meet.

The flat file's index is judged as test_gpu_writer_types.check_index judges it: tests/index_model.py for the types it knows
(test_gpu_writer_index.check_index's model), tests/writer_types_model.py for Timestamp and Decimal128, which index_model does not
know, and for the DICTIONARY_V2 column the positions tests/writer_dict_model.py writes: PRESENT's, then the run-length positions of
DATA's ids, nothing for LENGTH or DICTIONARY_DATA.  Every row group is then sought through its positions as well."""
import decimal
import io

import numpy as np
import pyarrow as pa
import pyarrow.orc as po
import pytest

import gpu_util as G
import oracle_lib as O
import index_model as IM
import writer_dict_model as DM
import writer_nested_model as NM
import writer_types_model as TM
from orcfile import PRESENT, OrcFile
from orc_rust_amd import ArrowReaderBuilder, ArrowWriterBuilder
from test_gpu_writer_compression import check_chunked
from test_gpu_writer_index import _read, same_values
from test_gpu_writer_nested import check as nested_check, gpu_write as nested_write, readers as nested_readers
from writer_nested_model import ints, list_array, map_array, strings

pytestmark = pytest.mark.gpu

STRIDE = 1000


def flat_batch(n, rng):
    def m(p=0.15):
        return rng.random(n) < p
    few = np.array(["north", "south", "east", "west"])[rng.integers(0, 4, n)]
    cols = [
        ("bool", pa.array(rng.random(n) < 0.5, mask=m())),
        ("i8", pa.array(rng.integers(-128, 128, n).astype(np.int8), mask=m())),
        ("i16", pa.array(rng.integers(-30000, 30000, n).astype(np.int16), mask=m())),
        ("i32", pa.array(rng.integers(-1 << 31, 1 << 31, n).astype(np.int32), mask=m())),
        ("i64", pa.array(np.cumsum(rng.integers(0, 9, n)).astype(np.int64), mask=m())),
        ("f32", pa.array(rng.standard_normal(n).astype(np.float32), mask=m())),
        ("f64", pa.array(rng.standard_normal(n) * 1e6, mask=m())),
        ("few", pa.array(few.tolist(), type=pa.string(), mask=m())),                                   # 4 distinct: DICTIONARY_V2
        ("each", pa.array(["row-%07d" % i for i in rng.permutation(n)], type=pa.large_string(), mask=m())),  # all distinct: DIRECT_V2
        ("bin", pa.array([bytes(rng.integers(0, 256, int(k)).astype(np.uint8)) for k in rng.integers(0, 9, n)], type=pa.binary(), mask=m())),
        ("ts", pa.array(rng.integers(-10 ** 17, 10 ** 18, n), type=pa.timestamp("ns"), mask=m())),
        ("tz", pa.array(rng.integers(0, 10 ** 18, n), type=pa.timestamp("ns", tz="UTC"), mask=m())),
        ("dec", pa.array([decimal.Decimal(int(v)).scaleb(-2) for v in rng.integers(-10 ** 14, 10 ** 14, n)], type=pa.decimal128(15, 2), mask=m())),
    ]
    return pa.RecordBatch.from_arrays([c for _, c in cols], names=[k for k, _ in cols])


def write_flat(batches, comp):
    out = io.BytesIO()
    b = (ArrowWriterBuilder(out, batches[0].schema, ctx=G.ctx()).with_batch_size(1024).with_row_index_stride(STRIDE)
         .with_dictionary_key_size_threshold(0.5))
    if comp:
        b = b.with_compression(comp)
    w = b.try_build()
    w.write(batches[0])
    w.flush_stripe()
    w.write(batches[1])
    w.close()
    rows, counts = w.stripe_rows(), w.dictionary_counts()
    w.free()
    return out.getvalue(), rows, counts


def dictionary_positions(arr, has_present, raws, block_size):
    """writer_dict_model.py's positions of a DICTIONARY_V2 column (Utf8: ids of 4 bytes); raws: the compressed streams, or None"""
    valid = np.asarray(arr.is_valid()).astype(np.uint8)
    before = np.concatenate([[0], np.cumsum(valid)])
    ids = DM.dictionary_of(arr.drop_null().to_pylist())[1]
    ptab, dtab = IM.RunTable(IM.ByteRuns(), IM.msb_bytes(valid)), IM.RunTable(IM.Rle2Runs(4, False), ids)
    pmap, dmap = (IM.chunk_map(raws["PRESENT"], block_size), IM.chunk_map(raws["DATA"], block_size)) if raws else (None, None)
    out = []
    for r0 in range(0, len(arr), STRIDE):
        pos = []
        if has_present:
            u, cons = ptab.at(r0 // 8)
            pos += (list(pmap(u)) if pmap else [u]) + [cons, r0 % 8]
        u, cons = dtab.at(int(before[r0]))
        out.append(pos + (list(dmap(u)) if dmap else [u]) + [cons])
    return out


def check_flat_index(data, table, rows, dict_col):
    """test_gpu_writer_types.check_index, the root's column included; column `dict_col` is written DICTIONARY_V2"""
    O.lib()
    of = OrcFile(data)
    assert of.row_index_stride == STRIDE and [s.number_of_rows for s in of.stripes] == rows
    groups, stripes, whole = TM.model_groups(table, rows, STRIDE)
    cols = [table.column(i).combine_chunks() for i in range(table.num_columns)]
    names = {0: "PRESENT", 1: "DATA", 2: "LENGTH", 5: "SECONDARY"}
    at = 0
    for si, s in enumerate(of.stripes):
        for col in range(0, table.num_columns + 1):
            entries = TM.row_index_entries(of, s, col)
            assert len(entries) == len(groups[si])
            want_pos = None
            if col:
                raws = {names[k]: bytes(v) for (c, k), v in s.streams.items() if c == col and k in names} if of.compression else None
                model = dictionary_positions if col == dict_col else lambda a, p, r, b: TM.model_positions(a, p, STRIDE, r, b)
                want_pos = model(cols[col - 1].slice(at, s.number_of_rows), (col, PRESENT) in s.streams, raws, of.block_size)
            for g, (pos, st) in enumerate(entries):
                assert TM.IM.same_stats(st, groups[si][g][col]), (si, g, col, st, groups[si][g][col])
                if want_pos is not None:
                    assert pos == want_pos[g], (si, g, col, pos, want_pos[g])
                elif not col:
                    assert pos == []
        at += s.number_of_rows
    fstats, sstats = TM.file_statistics(of)
    assert len(sstats) == len(of.stripes)
    for si, ss in enumerate(sstats):
        for col in range(table.num_columns + 1):
            assert TM.IM.same_stats(ss[col], stripes[si][col]), (si, col, ss[col], stripes[si][col])
    for col in range(table.num_columns + 1):
        assert TM.IM.same_stats(fstats[col], whole[col]), (col, fstats[col], whole[col])


@pytest.mark.parametrize("comp", [None, "snappy"])
def test_flat_types_index_dictionary_two_stripes(comp):
    rng = np.random.default_rng(77)
    batches = [flat_batch(2500, rng), flat_batch(700, rng)]
    table = pa.Table.from_batches(batches)
    data, rows, counts = write_flat(batches, comp)
    assert rows == [2500, 700]                                # three row groups, the last partial; then one
    assert counts == {"dictionary": 2, "direct": 2}, counts  # `few` and `each`, in each stripe
    want = TM.read_types(table)
    assert po.ORCFile(io.BytesIO(data)).read().equals(want), "pyarrow.orc read back something else"
    check_flat_index(data, table, rows, dict_col=table.schema.get_field_index("few") + 1)
    # every row group found through its positions, the dictionary column's among them
    whole, _ = _read(data)
    assert whole.num_rows == 3200
    for r0, n in ((0, 1000), (1000, 1000), (2000, 500), (2500, 700)):
        sel = ([(r0, True)] if r0 else []) + [(n, False)] + ([(3200 - r0 - n, True)] if r0 + n < 3200 else [])
        got, groups = _read(data, selection=sel)
        assert groups == (1, 4) and same_values(got, whole.slice(r0, n)), r0
    assert whole.column("few").to_pylist() == want.column("few").to_pylist()
    assert write_flat(batches, comp)[0] == data


def nested_batch(n, rng):
    a = list_array(n, rng, ints(rng, np.int32, 0.1), nulls=0.2)
    keys = list_array(n, rng, lambda m: pa.array(["k%d" % x for x in rng.integers(0, 30, m)]), nulls=0.15)
    b = map_array(keys, pa.array(rng.integers(-1 << 40, 1 << 40, len(keys.values)), mask=rng.random(len(keys.values)) < 0.2))
    st = pa.StructArray.from_arrays([a, b], names=["a", "b"], mask=pa.array(rng.random(n) < 0.1))
    return pa.RecordBatch.from_arrays([st, pa.array(rng.integers(0, 1 << 50, n), mask=rng.random(n) < 0.1)], names=["st", "i"])


def test_struct_of_list_and_map_two_writes_lz4():
    rng = np.random.default_rng(78)
    whole = nested_batch(300, rng)
    a, b = whole.column(0).field("a"), whole.column(0).field("b")
    assert 0 in np.diff(np.asarray(a.offsets))[np.asarray(a.is_valid())] and 0 in np.diff(np.asarray(b.offsets))[np.asarray(b.is_valid())]  # an empty list, an empty map
    batches = [whole.slice(0, 170), whole.slice(170)]
    nested_check(batches, batch_size=64)  # the file is the model's (tests/writer_nested_model.py), pyarrow.orc reads the input back
    plain, rows0, _, _ = nested_write(batches, batch_size=64)
    got, rows, _, _ = nested_write(batches, batch_size=64, comp="lz4", block=4096)
    assert rows == rows0
    check_chunked(got, plain, "lz4", 4096)
    nested_readers(got, batches)
