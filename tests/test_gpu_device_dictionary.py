"""Dictionary columns with device output: the keys and the stripe's dictionary stay in HBM as torch tensors; gathered by the keys
with torch they rebuild the strings of the plain host read.  Nothing is copied to the host, and the tensors outlive the reader."""
import gc
import io

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch

from orc_rust_amd import capi
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.arrow_writer import ArrowWriterBuilder

pytestmark = pytest.mark.gpu

_CTX = {}


def ctx():
    if 0 not in _CTX:
        _CTX[0] = capi.Context(0)
    return _CTX[0]


def three_stripe_file():
    rng = np.random.default_rng(3)
    rows = 30000
    w = ["", "€ uro", "DELIVER IN PERSON", "MAIL", "x" * 300]
    vals = [None if rng.random() < 0.2 else w[int(rng.integers(0, len(w)))] for _ in range(rows)]
    schema = pa.schema([("s", pa.string()), ("x", pa.int64())])
    buf = io.BytesIO()
    w = ArrowWriterBuilder(buf, schema).with_dictionary_key_size_threshold(1.0).try_build()
    for k in range(3):
        lo, hi = k * rows // 3, (k + 1) * rows // 3
        w.write(pa.record_batch([pa.array(vals[lo:hi], pa.string()), pa.array(np.arange(lo, hi), pa.int64())], schema=schema))
        w.flush_stripe()
    w.close()
    data = buf.getvalue()
    assert orc.ORCFile(io.BytesIO(data)).nstripes == 3
    return data


def gather(keys, validity, offsets, data):
    """strings of the rows from the tensors alone: torch on the device, one copy of the gathered pieces for the comparison"""
    k = keys.long()
    start, end = offsets.long()[k], offsets.long()[k + 1]
    host = data.cpu().numpy().tobytes()
    valid = validity.cpu().numpy() if validity is not None else np.ones(len(k), bool)
    return [host[s:e].decode() if ok else None for s, e, ok in zip(start.cpu().tolist(), end.cpu().tolist(), valid)]


def test_device_dictionary_tensors_rebuild_the_plain_read_and_outlive_the_reader():
    data = three_stripe_file()
    plain = list(ArrowReaderBuilder.try_new(data, ctx()).with_batch_size(4096).build())
    r = ArrowReaderBuilder.try_new(data, ctx()).with_batch_size(4096).with_dictionary_columns(["s"]).with_device_output().build()
    kept = []
    dict_ptrs = set()
    for k, db in enumerate(r):
        col = db.column("s")
        assert col.type == pa.dictionary(pa.int32(), pa.string())
        assert col.values.dtype == torch.int32 and col.values.is_cuda and col.values.shape == (db.num_rows,)
        d = col.dictionary
        assert d.offsets.dtype == torch.int32 and d.offsets.is_cuda and d.data.dtype == torch.uint8 and d.data.is_cuda
        assert int(d.offsets[0]) == 0 and int(d.offsets[-1]) == d.data.shape[0]
        dict_ptrs.add(d.offsets.data_ptr())
        assert gather(col.values, col.validity, d.offsets, d.data) == plain[k].column("s").to_pylist(), k
        assert db.to_pyarrow().column("s").dictionary_decode().equals(plain[k].column("s")), k
        assert np.array_equal(db.column("x").values.cpu().numpy(), np.asarray(plain[k].column("x")))
        if k in (0, len(plain) - 1):
            kept.append((col.values, col.validity, d.offsets, d.data, col.values.clone(), d.offsets.clone(), d.data.clone(), plain[k].column("s").to_pylist()))
        db.release()
    assert k + 1 == len(plain)
    assert 3 <= len(dict_ptrs) < len(plain)  # one dictionary per stripe, shared by the stripe's batches
    assert r.d2h_bytes() == 0
    r.close()
    del r, db, col, d
    gc.collect()
    torch.cuda.synchronize()
    for values, validity, offsets, bytes_, values0, offsets0, bytes0, want in kept:
        assert torch.equal(values, values0) and torch.equal(offsets, offsets0) and torch.equal(bytes_, bytes0)
        assert gather(values, validity, offsets, bytes_) == want
