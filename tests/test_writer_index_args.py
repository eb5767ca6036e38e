"""ArrowWriterBuilder.with_row_index_stride's arguments, and the statistics model (tests/index_model.py) against numpy and
against what pyarrow's own writer records for the same table -- no GPU."""
import io
import math

import numpy as np
import pyarrow as pa
import pyarrow.orc as po
import pytest

import index_model as IM
from orcfile import OrcFile
from orc_rust_amd.arrow_writer import ArrowWriterBuilder


@pytest.mark.parametrize("bad", [-1, 1 << 31, 1.5, "10", None, True])
def test_stride_errors(bad):
    with pytest.raises(ValueError):
        ArrowWriterBuilder(io.BytesIO(), pa.schema([("a", pa.int64())])).with_row_index_stride(bad)


@pytest.mark.parametrize("good", [0, 1, 10000, (1 << 31) - 1, np.int64(8)])
def test_stride_values(good):
    b = ArrowWriterBuilder(io.BytesIO(), pa.schema([("a", pa.int64())])).with_row_index_stride(good)
    assert b._row_index_stride == int(good)


def test_model_against_numpy():
    rng = np.random.default_rng(1)
    x = rng.integers(-1000, 1000, 500)
    m = rng.random(500) < 0.3
    st = IM.column_stats(pa.array(x, mask=m))
    v = x[~m]
    assert st == {"n": len(v), "has_null": True, "int": (v.min(), v.max(), v.sum())}
    big = IM.column_stats(pa.array(np.array([(1 << 63) - 1, 5], dtype=np.int64)))
    assert big["int"][2] is None
    f = rng.standard_normal(300)
    d = IM.column_stats(pa.array(f))["double"]
    assert d[0] == f.min() and d[1] == f.max() and math.isclose(d[2], math.fsum(f), rel_tol=1e-12)
    assert "double" not in IM.column_stats(pa.array([1.0, float("nan")]))
    s = IM.column_stats(pa.array(["b", "a", None, "é" * 600]))
    assert s["string"][0] == b"a" and s["string"][1] is None and s["string"][3] == ("é" * 511 + "ê").encode()
    assert s["string"][4] == 2 + 1200
    odd = ("a" + "é" * 600).encode()  # (byte 1024 is a continuation byte: the bound backs off one byte)
    assert IM.lower_bound(odd) == ("a" + "é" * 511).encode() and len(IM.lower_bound(odd)) == 1023
    assert IM.upper_bound(odd) == ("a" + "é" * 510 + "ê").encode()
    assert IM.upper_bound(("z" + "\U0010ffff" * 300).encode()) == b"{"
    assert "string" not in IM.column_stats(pa.array(["\U0010ffff" * 300]))
    assert IM.column_stats(pa.array([True, False, True, None]))["bucket"] == [2]
    assert IM.column_stats(pa.array([None, None], type=pa.int32())) == {"n": 0, "has_null": True}


def test_model_against_pyarrow_writer():
    """pyarrow's writer (Apache ORC C++) records the same counts, has_null, integer statistics and true counts"""
    import oracle_lib as O
    O.lib()
    rng = np.random.default_rng(2)
    n, S = 25000, 3000
    t = pa.table({"i": pa.array(rng.integers(-99, 99, n), mask=rng.random(n) < 0.2),
                  "b": pa.array(rng.random(n) < 0.4, mask=rng.random(n) < 0.1),
                  "z": pa.array(np.zeros(n, dtype=np.int32), mask=np.arange(n) < 7000)})
    buf = io.BytesIO()
    po.write_table(t, buf, row_index_stride=S, compression="uncompressed", stripe_size=1 << 30)
    of = OrcFile(buf.getvalue())
    rows = [s.number_of_rows for s in of.stripes]
    groups, stripes, whole = IM.model_groups(t, rows, S)
    for si, s in enumerate(of.stripes):
        for col in range(1, 4):
            entries = IM.row_index_entries(of, s, col)
            assert len(entries) == len(groups[si]) > 0
            for g, (_, st) in enumerate(entries):
                want = groups[si][g][col]
                assert st["n"] == want["n"] and st["has_null"] == want["has_null"], (col, g)
                for k in ("int", "bucket"):
                    if k in want:
                        assert st[k] == want[k], (col, g, k)
