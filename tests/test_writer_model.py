"""The Python model of the reference's ArrowWriter (tests/writer_model.py) against an independent ORC reader (pyarrow.orc,
Apache ORC C++): what it writes reads back as its input.  CPU only: this pins the model's container and stripe cut, which
tests/test_gpu_writer.py then holds the device writer to byte for byte."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.orc as po
import pytest

import oracle_lib as O
import writer_model as WM


def _read(data):
    return po.ORCFile(io.BytesIO(data))


def _all_types(n, rng, nulls=False):
    def m(a):
        if not nulls:
            return a
        mask = rng.random(n) < 0.2
        return pa.array(a.to_pylist(), type=a.type, mask=mask)
    cols = {
        "b": m(pa.array(rng.random(n) < 0.5)),
        "i8": m(pa.array(rng.integers(-128, 128, n).astype(np.int8))),
        "i16": m(pa.array(rng.integers(-3000, 3000, n).astype(np.int16))),
        "i32": m(pa.array(np.repeat(rng.integers(-1 << 20, 1 << 20, n // 4 + 1), 4)[:n].astype(np.int32))),
        "i64": m(pa.array(np.cumsum(rng.integers(0, 9, n)).astype(np.int64))),
        "f32": m(pa.array(rng.random(n).astype(np.float32))),
        "f64": m(pa.array(rng.random(n))),
        "s": m(pa.array(["v%d" % (x % 17) * int(x % 3) for x in range(n)])),
        "bin": m(pa.array([bytes([x % 251]) * (x % 5) for x in range(n)], type=pa.binary())),
    }
    return pa.RecordBatch.from_pydict(cols)


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("batch_size,sbs", [(1024, 64 << 20), (7, 256), (100, 4096)])
def test_model_round_trip(nulls, batch_size, sbs):
    O.lib()
    rng = np.random.default_rng(batch_size + nulls)
    batch = _all_types(3000, rng, nulls)
    data, rows = WM.write_model([batch], batch_size=batch_size, stripe_byte_size=sbs)
    f = _read(data)
    assert f.nrows == 3000 and f.nstripes == len(rows)
    assert f.read().equals(pa.Table.from_batches([batch]))
    if sbs < 64 << 20:
        assert len(rows) > 1


def test_model_small_stripes():
    """arrow_writer.rs test_write_small_stripes: 1 000 000 Int64 0..n, stripe_byte_size 256 -> more than one stripe."""
    n = 1_000_000
    batch = pa.RecordBatch.from_pydict({"x": pa.array(np.arange(n, dtype=np.int64))})
    data, rows = WM.write_model([batch], stripe_byte_size=256)
    f = _read(data)
    assert f.nstripes == len(rows) > 1 and sum(rows) == n
    assert f.read().column(0).to_numpy().tolist() == list(range(n))


def test_model_zero_stripes_and_empty_flush():
    schema = pa.schema([("a", pa.int64()), ("s", pa.string())])
    data, rows = WM.write_model([pa.RecordBatch.from_pydict({"a": pa.array([], pa.int64()), "s": pa.array([], pa.string())}, schema=schema)])
    assert rows == []
    f = _read(data)
    assert f.nrows == 0 and f.nstripes == 0
    # a stripe of 0 rows from flush_stripe() between writes
    b = pa.RecordBatch.from_pydict({"a": pa.array([1, 2, None]), "s": pa.array(["x", None, "zz"])}, schema=schema)
    data, rows = WM.write_model([b, b], flush_after=(0,), schema=schema)
    assert rows == [3, 3]
    assert _read(data).read().equals(pa.Table.from_batches([b, b]))


def test_model_sticky_present():
    """A validity buffer that first arrives in a later stripe: the PRESENT stream stays for the stripes after it."""
    schema = pa.schema([("a", pa.int32())])
    plain = pa.RecordBatch.from_pydict({"a": pa.array(np.arange(500, dtype=np.int32))}, schema=schema)
    nullable = pa.RecordBatch.from_pydict({"a": pa.array([1, None, 3] * 100, pa.int32())}, schema=schema)
    data, rows = WM.write_model([plain, nullable, plain], batch_size=64, stripe_byte_size=256)
    assert len(rows) > 2
    assert _read(data).read().equals(pa.Table.from_batches([plain, nullable, plain]))


def test_model_runs_self_check():
    """Both state machines: the runs they write out, strung together with what finish() writes, are the oracle's whole-stream
    bytes (values with every kind of run, every length class, and every end state)."""
    rng = np.random.default_rng(5)
    v = np.concatenate([np.full(700, 3), rng.integers(0, 1 << 40, 600), np.repeat(rng.integers(0, 5, 300), 3), np.arange(1100), [7, 7]]).astype(np.int64)
    for tail in ([], [9], [9, 9, 9], [1, 2, 3, 4]):
        vv = np.concatenate([v, np.array(tail, dtype=np.int64)])
        m = WM.RleV2Model(8, True)
        for x in vv.tolist():
            m.push(x)
        assert len(m.runs) > 10
        assert b"".join(m.runs) + m.finish() == O.enc_rle2(vv, 8, True)
    bv = np.concatenate([np.full(300, 1), rng.integers(0, 256, 400), np.repeat(rng.integers(0, 3, 90), 4), [5, 5], np.full(131, 2), [8]]).astype(np.uint8)
    for tail in ([], [4], [4, 4, 4], list(range(130))):
        vv = np.concatenate([bv, np.array(tail, dtype=np.uint8)])
        b = WM.ByteRleModel()
        for x in vv.tolist():
            b.push(x)
        assert len(b.runs) > 10 and b.emitted == sum(len(r) for r in b.runs)
        assert b"".join(b.runs) + b.finish() == O.enc_byte_rle(vv)
