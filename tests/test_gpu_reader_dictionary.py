"""Dictionary output on the GPU: ArrowReaderBuilder.with_dictionary_columns / ORCGPU_ARROW_DICTIONARY_UTF8.

The judge is never the new code: pyarrow.orc's read of the same file, and this reader's own plain Utf8 read under the same
options (what the reader did before the option existed).  A dictionary column, dictionary_decode()d, must be the plain column
batch for batch, with the plain read's batch boundaries.  On top: the type, the dictionary against the file's own entries and the
keys against its DATA ids (tests/orcfile.py + the oracle's RLE decoders), one dictionary per stripe, and fewer bytes copied back."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded)

import oracle_lib as O
import orcfile
from orc_rust_amd import capi, gen
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.arrow_writer import ArrowWriterBuilder
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

pytestmark = pytest.mark.gpu

DICT_T = pa.dictionary(pa.int32(), pa.string())
_CTX = {}


def ctx():
    if 0 not in _CTX:
        _CTX[0] = capi.Context(0)
    return _CTX[0]


def read(source, dict_cols=None, batch_size=1000, prefetch=0, **opts):
    b = ArrowReaderBuilder.try_new(source, ctx()).with_batch_size(batch_size).with_prefetch(prefetch)
    if opts.get("projection") is not None:
        b = b.with_projection(opts["projection"])
    if opts.get("selection") is not None:
        b = b.with_row_selection(opts["selection"])
    if opts.get("predicate") is not None:
        b = b.with_predicate(opts["predicate"])
    if opts.get("row_filter") is not None:
        b = b.with_row_filter(opts["row_filter"], prune=False)
    if dict_cols is not None:
        b = b.with_dictionary_columns(dict_cols)
    r = b.build()
    out = list(r)
    d2h = r.d2h_bytes()
    r.close()
    return out, d2h


def check(source, dict_cols, batch_size=1000, judge=True, **opts):
    """The dictionary read against the plain read (and, without options that change the rows, against pyarrow.orc).  Returns the
    dictionary read's batches and both d2h byte counts."""
    plain, d2h_plain = read(source, None, batch_size, **opts)
    got, d2h_dict = read(source, dict_cols, batch_size, **opts)
    assert len(got) == len(plain), (len(got), len(plain))
    for k, (g, p) in enumerate(zip(got, plain)):
        g.validate(full=True)
        assert g.num_rows == p.num_rows and g.schema.names == p.schema.names, k
        for name in p.schema.names:
            gc, pc = g.column(name), p.column(name)
            if name in dict_cols:
                assert gc.type == DICT_T, (k, name, gc.type)
                assert pc.type == pa.string()
                assert gc.null_count == pc.null_count
                assert gc.dictionary_decode().equals(pc), (k, name)
                # a null row's key is 0
                keys = np.asarray(gc.indices.fill_null(0)) if gc.null_count else np.asarray(gc.indices)
                raw = np.frombuffer(gc.indices.buffers()[1], dtype=np.int32, count=len(gc))
                assert np.array_equal(raw, keys), (k, name)
            else:
                assert gc.equals(pc), (k, name)  # the other columns stay bit-identical
    if judge and not any(opts.get(o) is not None for o in ("selection", "predicate", "row_filter")):
        want = orc.read_table(io.BytesIO(source) if isinstance(source, bytes) else source, columns=opts.get("projection"))
        for name in dict_cols if got else []:
            # (a batch without nulls is exported as not nullable, as on the plain path: the columns are put together, not the schemas)
            mine = pa.chunked_array([g.column(name).dictionary_decode() for g in got], pa.string())
            assert mine.combine_chunks().equals(want.column(name).cast(pa.string()).combine_chunks()), name
    return got, d2h_dict, d2h_plain


def words(n_distinct):
    """n_distinct different strings: the empty one, one with a 3-byte UTF-8 character, plain ones"""
    base = ["", "€ uro", "DELIVER IN PERSON"]
    return (base + ["w%07d" % i for i in range(n_distinct)])[:n_distinct]


def string_table(rows, n_distinct, nulls=0.25, seed=1, long_entry=False):
    rng = np.random.default_rng(seed)
    w = words(n_distinct)
    if long_entry and n_distinct > 3:
        w[3] = "L" * 5000
    ids = np.concatenate([np.arange(n_distinct), rng.integers(0, n_distinct, max(0, rows - n_distinct))])[:rows]
    rng.shuffle(ids)
    mask = rng.random(rows) < nulls if nulls else np.zeros(rows, bool)
    if nulls >= 1.0:
        mask[:] = True
    else:
        mask[np.unique(ids, return_index=True)[1]] = False  # (every distinct value stays in the file)
    vals = [None if m else w[i] for i, m in zip(ids, mask)]
    return pa.table({"s": pa.array(vals, pa.string()), "x": pa.array(rng.integers(-1 << 40, 1 << 40, rows), pa.int64()),
                     "t": pa.array(["k%d" % (i % 3) for i in range(rows)], pa.string())})


def pyarrow_file(table, compression="uncompressed", stripe_size=None, **kw):
    buf = io.BytesIO()
    args = dict(dictionary_key_size_threshold=1.0, compression=compression)
    if compression != "uncompressed":
        args["compression_block_size"] = 65536
    if stripe_size:
        args["stripe_size"] = stripe_size
    args.update(kw)
    orc.write_table(table, buf, **args)
    return buf.getvalue()


def encodings(data, name):
    f = orcfile.OrcFile(data)
    cid = [c for n, c, _ in f.root_columns() if n == name][0]
    return f, cid, [s.encodings[cid] for s in f.stripes]


_FILES = {}


def rows_file(rows):
    if rows not in _FILES:
        _FILES[rows] = pyarrow_file(string_table(rows, min(rows, 11)))
    return _FILES[rows]


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000, 8193])
@pytest.mark.parametrize("batch_size", [1, 7, 100, 1024, 8192])
def test_rows_and_batch_sizes(rows, batch_size):
    check(rows_file(rows), ["s"], batch_size)


def test_type_file_order_dictionary_and_data_ids():
    """A dictionary-encoded stripe: the dictionary is the file's, entry for entry in file order, the keys are the DATA ids"""
    data = pyarrow_file(string_table(3000, 40, nulls=0.25, long_entry=True))
    f, cid, enc = encodings(data, "s")
    assert all(e[0] in (1, 3) for e in enc), enc
    got, _, _ = check(data, ["s", "t"], 1000)
    at = 0
    for si, s in enumerate(f.stripes):
        kind, dsz = s.encodings[cid]
        st = f.column_streams(s, cid)
        version = 2 if kind == 3 else 1
        rc, lens = O.int_rle(st[orcfile.LENGTH], dsz, version=version, signed=False)
        assert rc == 0
        blob = st[orcfile.DICTIONARY_DATA]
        offs = np.concatenate([[0], np.cumsum(lens)])
        entries = [blob[offs[k]:offs[k + 1]].decode() for k in range(dsz)]
        n_b = (s.number_of_rows + 999) // 1000
        batches = got[at:at + n_b]
        at += n_b
        nonnull = sum(len(b.column("s")) - b.column("s").null_count for b in batches)
        rc, ids = O.int_rle(st[orcfile.DATA], nonnull, version=version, signed=False)
        assert rc == 0
        seen = []
        for b in batches:
            col = b.column("s")
            assert col.type == DICT_T
            assert col.dictionary.to_pylist() == entries
            # all batches of one stripe share one dictionary: the same buffers
            assert [x.address for x in col.dictionary.buffers()[1:]] == [x.address for x in batches[0].column("s").dictionary.buffers()[1:]]
            seen += [k for k in col.indices.to_pylist() if k is not None]
        assert seen == ids.tolist()


@pytest.mark.parametrize("nulls", ["none", "quarter", "all", "runs"])
def test_nulls(nulls):
    rows = 1000
    if nulls == "runs":
        # a null run across a 64-row word and across a batch edge (batch size 100)
        vals = ["v%d" % (i % 5) for i in range(rows)]
        for a, b in ((60, 70), (95, 130), (192, 320)):
            vals[a:b] = [None] * (b - a)
        t = pa.table({"s": pa.array(vals, pa.string())})
    else:
        t = string_table(rows, 9, nulls={"none": 0, "quarter": 0.25, "all": 1.0}[nulls]).select(["s", "x"])
    data = pyarrow_file(t)
    got, _, _ = check(data, ["s"], 100)
    if nulls == "all":
        assert all(len(b.column("s").dictionary) == 0 for b in got)


@pytest.mark.parametrize("n_distinct", [1, 2, 254, 255, 256, 257, 65535, 65537])
def test_dictionary_sizes_and_key_widths(n_distinct):
    rows = n_distinct + 700
    data = pyarrow_file(string_table(rows, n_distinct, nulls=0.1).select(["s"]), stripe_size=64 << 20)
    _, _, enc = encodings(data, "s")
    assert enc[0][0] in (1, 3) and enc[0][1] == n_distinct, enc
    got, _, _ = check(data, ["s"], 8192)
    assert len(got[0].column("s").dictionary) == n_distinct


def test_our_writer_unsorted_dictionaries_and_mixed_encodings():
    """Our writer chooses per stripe: at threshold 0.5 a stripe of few distinct values is DICTIONARY_V2 (unsorted, first occurrence),
    one of all-distinct values DIRECT_V2, which shows the identity dictionary with ascending keys"""
    schema = pa.schema([("s", pa.string()), ("x", pa.int64())])
    n = 2000
    lo = pa.record_batch([pa.array([None if i % 7 == 0 else "z%d" % (9 - i % 10) for i in range(n)], pa.string()), pa.array(range(n), pa.int64())], schema=schema)
    hi = pa.record_batch([pa.array([None if i % 5 == 0 else "u%06d" % (n - i) for i in range(n)], pa.string()), pa.array(range(n), pa.int64())], schema=schema)
    buf = io.BytesIO()
    w = ArrowWriterBuilder(buf, schema).with_dictionary_key_size_threshold(0.5).try_build()
    w.write(lo)
    w.flush_stripe()
    w.write(hi)
    w.close()
    data = buf.getvalue()
    _, _, enc = encodings(data, "s")
    assert [e[0] for e in enc] == [3, 2], enc
    got, _, _ = check(data, ["s"], 1000)
    first, direct = got[0].column("s"), got[2:]
    assert first.dictionary.to_pylist()[:3] == ["z8", "z7", "z6"]  # first occurrence, not sorted
    keys = [k for b in direct for k in b.column("s").indices.to_pylist() if k is not None]
    assert keys == list(range(len(keys)))
    assert len(direct[0].column("s").dictionary) == len(keys)


@pytest.mark.parametrize("compression", ["uncompressed", "snappy", "zlib", "zstd"])
def test_compressions(compression):
    check(pyarrow_file(string_table(8193, 300, long_entry=True), compression), ["s", "t"], 1024)


def test_projection_that_drops_columns():
    check(rows_file(1000), ["s"], 100, projection=["s", "x"])
    check(rows_file(1000), ["t"], 100, projection=["x", "t"])


def test_d2h_bytes_are_fewer():
    t = string_table(5000, 16, nulls=0).select(["t"])
    _, d2h_dict, d2h_plain = check(pyarrow_file(t), ["t"], 1024)
    assert 0 < d2h_dict < d2h_plain, (d2h_dict, d2h_plain)


def indexed_file():
    t = string_table(30000, 50, nulls=0.2)
    t = t.set_column(1, "x", pa.array(np.arange(30000), pa.int64()))
    return pyarrow_file(t, row_index_stride=1000, stripe_size=64 << 20)


def test_row_selection_predicate_filter_prefetch():
    data = indexed_file()
    sel = [(37, True), (100, False), (1900, True), (64, False), (3000, True), (5001, False)]
    check(data, ["s"], 1000, selection=sel)
    check(data, ["s", "t"], 1000, predicate=P.gt("x", V.Int64(21500)))
    got, _, _ = check(data, ["s"], 1000, row_filter=P.and_([P.gte("x", V.Int64(777)), P.lt("x", V.Int64(9123))]))
    assert sum(b.num_rows for b in got) == 9123 - 777
    check(data, ["s"], 1000, prefetch=2)


def test_a_row_filter_on_the_dictionary_column_is_refused():
    data = rows_file(1000)
    b = ArrowReaderBuilder.try_new(data, ctx()).with_prefetch(0).with_dictionary_columns(["s"])
    r = b.with_row_filter(P.eq("s", V.Utf8("w0000003")), prune=False).build()
    with pytest.raises(capi.OrcGpuError) as e:
        next(r)
    assert e.value.code == 7 and "'s'" in str(e.value), str(e.value)
    r.close()


def test_reader_refuses_bad_names():
    data = rows_file(1000)
    for names, word in ((["nope"], "nope"), (["x"], "x")):
        b = ArrowReaderBuilder.try_new(data, ctx())
        with pytest.raises(capi.OrcGpuError) as e:
            b.with_dictionary_columns(names)
        assert e.value.code == 101 and word in str(e.value)


# ---- the C ABI: hand-built stripes ------------------------------------------------------------------------------------------
def dict_stripe(ids, entries, dictionary_size=None, present=None):
    blob = b"".join(entries)
    col = {"column_id": 1, "orc_type": 7, "encoding": 3, "dictionary_size": len(entries) if dictionary_size is None else dictionary_size}
    streams = [(1, 1, gen.rle2(np.asarray(ids, np.int64), signed=False)), (1, 2, gen.rle2(np.asarray([len(e) for e in entries], np.int64), signed=False)),
               (1, 3, np.frombuffer(blob, np.uint8))]
    if present is not None:
        streams.insert(0, (1, 0, gen.boolean(np.asarray(present, np.uint8))))
    return col, streams


def decode(n, col, streams, target, batch_size=100):
    c = dict(col)
    c["arrow_target"] = target
    staged = ctx().stage(n, streams, [c], batch_size=batch_size)
    res = ctx().decode([staged])[0]
    staged.free()
    return res


def decoded_strings(res, b, target):
    v = res.batch(b, 0)
    valid = np.ones(v["length"], bool) if v["validity"] is None else np.unpackbits(np.frombuffer(v["validity"], np.uint8), bitorder="little")[:v["length"]].astype(bool)
    if target == 27:
        assert v["offsets"] is None and len(v["values"]) == 4 * v["length"]
        keys = np.frombuffer(v["values"], np.int32)
        assert not keys[~valid].any()
        offs, blob = res.dictionary(0)
        return [blob[offs[k]:offs[k + 1]] if ok else None for k, ok in zip(keys, valid)]
    o = v["offsets"]
    return [v["values"][o[i]:o[i + 1]] if valid[i] else None for i in range(v["length"])]


def test_abi_bad_id_fails_the_same_batch_as_utf8():
    rng = np.random.default_rng(5)
    entries = [b"a", b"", b"ccc", "€".encode(), b"e" * 40]
    present = rng.random(300) > 0.2
    ids = rng.integers(0, 5, int(present.sum()))
    k = int(present[:150].sum())  # the id of row 150: batch 1
    ids[k] = 5
    col, streams = dict_stripe(ids, entries, present=present)
    plain, dic = decode(300, col, streams, 0), decode(300, col, streams, 27)
    assert plain.status() == dic.status() and dic.status()[0] == 8 and dic.status()[1] == 1, (plain.status(), dic.status())
    assert decoded_strings(dic, 0, 27) == decoded_strings(plain, 0, 0)
    plain.free()
    dic.free()


def test_abi_good_stripe_and_struct_field():
    entries = [b"a", b"", b"ccc", "€".encode()]
    ids = np.arange(300) % 4
    col, streams = dict_stripe(ids, entries)
    plain, dic = decode(300, col, streams, 0), decode(300, col, streams, 27)
    assert dic.status()[0] == 0
    for b in range(3):
        assert decoded_strings(dic, b, 27) == decoded_strings(plain, b, 0)
    plain.free()
    dic.free()
    # a string field of a Struct root
    cols = [{"column_id": 1, "orc_type": 12, "encoding": 0}, dict(col, column_id=2, parent=1, arrow_target=27)]
    sp = (np.arange(300) % 3 != 0)
    ids2 = (np.arange(int(sp.sum())) % 4)
    st = [(1, 0, gen.boolean(sp.astype(np.uint8))), (2, 1, gen.rle2(ids2.astype(np.int64), signed=False)),
          (2, 2, gen.rle2(np.asarray([len(e) for e in entries], np.int64), signed=False)), (2, 3, np.frombuffer(b"".join(entries), np.uint8))]
    staged = ctx().stage(300, st, cols, batch_size=100)
    res = ctx().decode([staged])[0]
    staged.free()
    assert res.status()[0] == 0, res.status()
    rb = res.export_batch(0)
    f = rb.column(0).field(0)
    assert f.type == DICT_T
    want = [entries[k % 4].decode() for k in range(int(sp[:100].sum()))]
    assert [x for x in f.dictionary_decode().to_pylist() if x is not None] == want
    res.free()


def test_abi_invalid_utf8_entry_and_other_types():
    entries = [b"a", b"\xff\xfe", b"c"]
    col, streams = dict_stripe(np.arange(300) % 3, entries)
    plain, dic = decode(300, col, streams, 0), decode(300, col, streams, 27)
    assert plain.status() == dic.status() and dic.status()[0] == 8, (plain.status(), dic.status())
    plain.free()
    dic.free()
    icol = {"column_id": 1, "orc_type": 4, "encoding": 2}
    ist = [(1, 1, gen.rle2(np.arange(300, dtype=np.int64), signed=True))]
    codes = []
    for target in (17, 27):
        with pytest.raises(capi.OrcGpuError) as e:
            decode(300, icol, ist, target)
        codes.append(e.value.code)
    assert codes == [6, 6]
