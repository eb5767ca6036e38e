"""The row index model's positions (tests/index_model.py) without a GPU: every stream of every row group is decoded by the
oracle's decoders from the group's entry alone -- uncompressed, and with each stream chunked as Snappy and LZ4 -- and must give
the group's values."""
import numpy as np
import pyarrow as pa
import pytest

import index_model as IM
import oracle_lib as O
import writer_model as WM
from orcfile import OrcFile, PRESENT


def _table(n, rng):
    m = rng.random(n) < 0.3
    return pa.table({
        "i64": pa.array(np.repeat(rng.integers(-9, 9, n // 5 + 1), 5)[:n], mask=m),
        "i8": pa.array(rng.integers(-128, 128, n).astype(np.int8)),
        "i16": pa.array(np.arange(n).astype(np.int16) % 300),
        "f32": pa.array(rng.standard_normal(n).astype(np.float32), mask=rng.random(n) < 0.5),
        "f64": pa.array(rng.standard_normal(n)),
        "b": pa.array(rng.random(n) < 0.3, mask=rng.random(n) < 0.2),
        "s": pa.array(["v%d" % (x % 37) for x in range(n)], mask=m),
        "ls": pa.array(["w" * (x % 5) for x in range(n)], type=pa.large_string()),
        "bin": pa.array([b"\x00" * (x % 3) for x in range(n)], type=pa.binary(), mask=rng.random(n) < 0.1),
        "lbin": pa.array([b"q" * (x % 7) for x in range(n)], type=pa.large_binary()),
    })


def _chunked(raw, codec, block):
    """a stream as the writer chunks it: blocks of `block` bytes, each compressed, or original when that is not smaller"""
    out = bytearray()
    for at in range(0, len(raw), block):
        b = raw[at:at + block]
        z = pa.Codec(codec).compress(b, asbytes=True) if codec else b
        if codec and len(z) < len(b):
            h = len(z) * 2
            out += bytes([h & 255, (h >> 8) & 255, h >> 16]) + z
        else:
            h = len(b) * 2 + 1
            out += bytes([h & 255, (h >> 8) & 255, h >> 16]) + b
    return bytes(out)


def _from_entry(raw, pos, comp, block):
    """the stream's bytes from an entry's first numbers on, and the rest of the entry"""
    if comp is None:
        return raw[pos[0]:], pos[1:]
    st, plain = O.stream_decompress(raw[pos[0]:], comp, block)
    assert st == 0
    return plain[pos[1]:], pos[2:]


def _bits(data, skip_bytes, skip_bits, n):
    nb = (skip_bits + n + 7) // 8
    st, b = O.byte_rle(data, skip_bytes + nb)
    assert st == 0
    return np.unpackbits(b[skip_bytes:].view(np.uint8), bitorder="big")[skip_bits:skip_bits + n]


@pytest.mark.parametrize("comp", [None, "snappy", "lz4"])
@pytest.mark.parametrize("stride", [1, 7, 8, 1000])
def test_positions_decode_every_group(comp, stride):
    O.lib()
    rng = np.random.default_rng(stride)
    n = 200 if stride < 8 else 5000
    t = _table(n, rng)
    data, rows = WM.write_model(t.to_batches(max_chunksize=1500), batch_size=70 if n < 1000 else 700, stripe_byte_size=(1 << 10) if n < 1000 else 16 << 10)
    of = OrcFile(data)
    codec, block = {None: (None, 0), "snappy": ("snappy", 1000), "lz4": ("lz4_raw", 777)}[comp]
    at = 0
    checked = 0
    for s in of.stripes:
        R = s.number_of_rows
        for ci, name in enumerate(t.column_names):
            col = ci + 1
            arr = t.column(name).combine_chunks().slice(at, R)
            has_present = (col, PRESENT) in s.streams
            w, valid, streams = IM.column_streams(arr, has_present)
            raws = {k: bytes(s.streams[(col, {"PRESENT": 0, "DATA": 1, "LENGTH": 2}[k])]) for k, _, _ in streams}
            if comp:
                raws = {k: _chunked(v, codec, block) for k, v in raws.items()}
            entries = IM.model_positions(arr, has_present, stride, raws if comp else None, block or 262144)
            assert len(entries) == (R + stride - 1) // stride
            before = np.concatenate([[0], np.cumsum(valid)])
            for g, pos in enumerate(entries):
                r0, r1 = g * stride, min(R, (g + 1) * stride)
                v0, v1 = int(before[r0]), int(before[r1])
                for kind, form, vals in streams:
                    k = r1 - r0 if kind == "PRESENT" else v1 - v0
                    want = vals[r0:r1] if kind == "PRESENT" else vals[v0:v1]
                    d, rest = _from_entry(raws[kind], pos, comp, block or 262144)
                    pos = rest[(1 if form >= 2 else 0) + (1 if form == 3 else 0):]
                    if not k:
                        continue
                    if form == 3:
                        got = _bits(d, rest[0], rest[1], k)
                    elif kind == "LENGTH":
                        st, got = O.int_rle(d, rest[0] + k, signed=False)
                        got = got[rest[0]:]
                    elif form == 2 and w == "byte":
                        st, got = O.byte_rle(d, rest[0] + k)
                        got = got[rest[0]:].view(np.uint8)
                    elif form == 2:
                        st, got = O.int_rle(d, rest[0] + k, signed=True)
                        got = got[rest[0]:]
                    elif w == "str":
                        got = np.frombuffer(d[:int(want.sum())], dtype=np.uint8)
                        flat = [x.encode() if isinstance(x, str) else x for x in arr.drop_null().to_pylist()[v0:v1]]
                        want = np.frombuffer(b"".join(flat), dtype=np.uint8)
                    else:
                        got = np.frombuffer(d[:k * want.dtype.itemsize], dtype=want.dtype)
                    np.testing.assert_array_equal(np.asarray(got), np.asarray(want), err_msg="%s %s group %d" % (name, kind, g))
                    checked += 1
                assert pos == [], (name, g, pos)
        at += R
    assert len(of.stripes) >= 2 and checked > 0
