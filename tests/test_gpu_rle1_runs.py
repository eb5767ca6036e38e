"""The HIP integer RLE v1, byte RLE and boolean decoders on the hand-built runs of tests/test_rle1_cases.py (written with
tests/rle1_enc.py): forms no encoder of this project emits, placed where the scan pass (device/rle_scan.hip) cuts the stream -- at
block offsets 0, 1, 510 and 511 of a 512-byte block, across span (256 blocks) and tile (1024 blocks) boundaries, alone, behind
valid runs and in front of them, at batch sizes 8192, 1000, 7 and 1 -- against the oracle (G.assert_column_parity) AND against the
tables' values, which the plain model reproduces (test_rle1_cases).  Then the walk's paths, and which of them ran: a child process
under ORCGPU_DEBUG whose per-job lines are read.

Carriers: signed RLE v1 is the DATA stream of a Long / Int / Short column of encoding 0 (N = i64 / i32 / i16); unsigned RLE v1 the
LENGTH stream of a Binary column of encoding 0 -- the cases whose values can be lengths (0 .. 1000); the others are judged off the
GPU only --, and the DATA stream of a dictionary column of encoding 1 (the 64-bit decoder with 32-bit keys); byte RLE a Byte
column; booleans the DATA of a Boolean column and the PRESENT of a Long column.  A failing column ends the stripe (one status per
result), so every malformed case is a call of its own."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gpu_util as G
import rle1_enc as E
import test_rle1_cases as T
from rle1_enc import BOOL, BYTE, V1

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RLE_BLK, SPAN, TILE = 512, 256 * 512, 1024 * 512
TYPES = {(V1, 64): (4, np.int64), (V1, 32): (3, np.int32), (V1, 16): (2, np.int16), (BYTE, 8): (1, np.int8), (BOOL, 8): (0, np.uint8)}
CARRIERS = sorted(TYPES, key=str)
BINARY, STRING, PRESENT, DATA, LENGTH, DICT = 8, 7, 0, 1, 2, 3
FULL_BYTES = [(i * 5) % 100 for i in range(128)]
# a full group per codec: 128 literals (RLE v1: one-byte varints, signed), 129 bytes; a boolean one is 1024 bits
FULL = {V1: (E.v1_literals([(b >> 1) ^ -(b & 1) for b in FULL_BYTES], True), [(b >> 1) ^ -(b & 1) for b in FULL_BYTES]),
        BYTE: (E.byte_literals(FULL_BYTES), FULL_BYTES), BOOL: (E.byte_literals(FULL_BYTES), [(b >> (7 - k)) & 1 for b in FULL_BYTES for k in range(8)])}
PER_FULL = {V1: 128, BYTE: 128, BOOL: 1024}


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def col(cid, codec, nbits):
    return {"column_id": cid, "orc_type": TYPES[(codec, nbits)][0], "encoding": 0}


def values_of(res, ci, codec, nbits, batches=None):
    dtype = TYPES[(codec, nbits)][1]
    out = []
    for b in range(res.n_batches if batches is None else batches):
        g = res.batch(b, ci)
        v = np.frombuffer(g["values"], dtype=dtype)
        out.append(np.unpackbits(v, bitorder="little")[:g["length"]] if codec == BOOL else v)  # (a Boolean column's values: an Arrow bitmap)
    return np.concatenate(out or [np.zeros(0, dtype)])


def filler(codec, k):
    """valid runs of exactly k bytes (k >= 2): full groups, then one or two literal groups that take the rest; (bytes, values)"""
    nfull = (k - 131 + 128) // 129 if k > 131 else 0
    out, vals, k = FULL[codec][0] * nfull, FULL[codec][1] * nfull, k - 129 * nfull
    for part in ((k,) if k <= 129 else (65, k - 65)):
        g = FULL_BYTES[:part - 1]
        out += E.byte_literals(g)  # (one-byte varints: the same bytes in RLE v1)
        vals += FULL[codec][1][:(part - 1) * (8 if codec == BOOL else 1)]
    return out, vals


def to_offset(codec, at, offset, modulus=RLE_BLK):
    """filler that brings a stream of `at` bytes to `offset` modulo `modulus`"""
    k = (offset - at) % modulus
    return filler(codec, k if k >= 2 else k + modulus) if k else (b"", [])


def cases(codec, nbits):
    """the table's cases for a carrier (signed ones for RLE v1); a boolean case's values reach to the end of its last byte, whose
    unused bits the table sets -- but for the cases with more in the stream, which stand alone"""
    out = []
    for name, (c, stream, want, signed, n) in T.VALID.items():
        if (c, n) == (codec, nbits) and (signed or codec != V1):
            if codec == BOOL and not name.endswith("more in the stream than asked"):
                want = want + [1] * (-len(want) % 8)
            out.append((name, stream, want))
    return out


def check_column(res, ci, c, streams, n, batch, want, codec, nbits, what):
    assert res.status()[0] == 0, (what, res.status())
    got = values_of(res, ci, codec, nbits).tolist()
    if got != want:
        bad = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b) if len(got) == len(want) else -1
        raise AssertionError((what, "first wrong value", bad, len(got), len(want)))
    G.assert_column_parity(res, ci, c, streams, n, batch, what=what)


@pytest.mark.parametrize("codec,nbits", CARRIERS)
def test_valid_cases_alone(codec, nbits):
    """every case a column of its own, 600 columns a call.  A column has the stripe's row count: full groups stand behind the
    shorter cases -- in FRONT of them for the byte cases named `last`, whose run must stay the stream's last (the full parse of
    hop_parse<CODEC_BYTE>, which the 129 last bytes of a stream take)"""
    per, (full, fullv) = PER_FULL[codec], FULL[codec]
    all_cases = [c for c in cases(codec, nbits) if not c[0].endswith("more in the stream than asked")]
    for part in range(0, len(all_cases), 600):
        chunk = all_cases[part:part + 600]
        n = max(len(c[2]) for c in chunk) + per
        cols, streams, wants = [], [], []
        for i, (name, stream, want) in enumerate(chunk):
            pad = (n - len(want) + per - 1) // per
            cols.append(col(i + 1, codec, nbits))
            if name.endswith("/last"):
                head = (pad * per - (n - len(want)))  # values of the padding that are cut off its front: a shorter first group
                front = E.byte_literals(FULL_BYTES[head:]) + full * (pad - 1)
                streams.append((i + 1, DATA, u8(front + stream)))
                wants.append(fullv[head:] + fullv * (pad - 1) + want)
                assert len(wants[-1]) == n
            else:
                streams.append((i + 1, DATA, u8(stream + full * pad)))
                wants.append((want + fullv * pad)[:n])
        for batch in (8192, 1000):
            res = G.gpu_decode(n, cols, streams, batch_size=batch)
            for ci, c in enumerate(cols):
                check_column(res, ci, c, streams, n, batch, wants[ci], codec, nbits, (chunk[ci][0], batch))
            res.free()


def test_boolean_streams_that_hold_more_than_is_asked():
    """each alone, its row count the bits asked: what the stream holds behind them is never looked at"""
    for name, (c, stream, want, _s, _n) in T.VALID.items():
        if name.endswith("more in the stream than asked"):
            cc, s = col(1, BOOL, 8), [(1, DATA, u8(stream))]
            for batch in (8192, 7):
                res = G.gpu_decode(len(want), [cc], s, batch_size=batch)
                check_column(res, 0, cc, s, len(want), batch, want, BOOL, 8, (name, batch))
                res.free()


def test_boolean_cases_as_present_streams():
    """the boolean cases as the PRESENT stream of a Long column whose DATA is plain full groups: validity is the case's bits"""
    chunk = [c for c in cases(BOOL, 8) if not c[0].endswith("more in the stream than asked")]
    n = max(len(c[2]) for c in chunk)
    cols, streams, wants = [], [], []
    for i, (name, stream, want) in enumerate(chunk):
        pad = (n - len(want) + 1023) // 1024
        bits = (want + FULL[BOOL][1] * pad)[:n]
        cols.append(col(i + 1, V1, 64))
        streams += [(i + 1, PRESENT, u8(stream + FULL[BOOL][0] * pad)), (i + 1, DATA, u8(FULL[V1][0] * (sum(bits) // 128 + 1)))]
        wants.append(bits)
    for batch in (8192, 1000):
        res = G.gpu_decode(n, cols, streams, batch_size=batch)
        assert res.status()[0] == 0, res.status()
        for ci, c in enumerate(cols):
            got = []
            for b in range(res.n_batches):
                g = res.batch(b, ci)
                got += [1] * g["length"] if g["validity"] is None else np.unpackbits(np.frombuffer(g["validity"], dtype=np.uint8), bitorder="little")[:g["length"]].tolist()
            assert got == wants[ci], (chunk[ci][0], batch)
            G.assert_column_parity(res, ci, c, streams, n, batch, what=(chunk[ci][0], batch))
        res.free()


@functools.lru_cache(maxsize=None)
def one_stream(codec, nbits, offset):
    """every case's first byte at block offset `offset`, fillers between them and full groups behind the last"""
    out, vals = bytearray(FULL[codec][0]), list(FULL[codec][1])
    for name, stream, want in cases(codec, nbits):
        if name.endswith(("/last", "more in the stream than asked")):
            continue
        f, fv = to_offset(codec, len(out), offset)
        out += f + stream
        vals += fv + want
    # 2048 blocks and more: the call passes the gate of the exact parallel walk (the boolean cases -- CODEC_BYTE once more, eight
    # rows a byte -- stay as short as they are)
    more = max(0, (2049 * RLE_BLK - len(out)) // 129 + 1) if codec != BOOL else 1
    return bytes(out) + FULL[codec][0] * more, vals + FULL[codec][1] * more


@pytest.mark.parametrize("offset", [0, 1, 510, 511])
@pytest.mark.parametrize("codec,nbits", CARRIERS)
def test_valid_cases_in_one_stream_at_block_offsets(codec, nbits, offset):
    """all cases of one carrier in ONE stream of about 1.1 MiB, each case's header at the same offset of a block: the runs' payloads
    lie across block boundaries all over (the 1281-byte literal group from offset 511: two blocks pure pass-through, its end in a
    third), every case has valid runs in front and behind"""
    stream, want = one_stream(codec, nbits, offset)
    assert (2048 * RLE_BLK if codec != BOOL else 64 * RLE_BLK) < len(stream) < 4 << 20, len(stream)
    c, s = col(1, codec, nbits), [(1, DATA, u8(stream))]
    for batch in (8192, 1000):
        res = G.gpu_decode(len(want), [c], s, batch_size=batch)
        check_column(res, 0, c, s, len(want), batch, want, codec, nbits, (codec, nbits, offset, batch))
        res.free()


def straddlers(codec):
    """the long cases: their payloads are what can lie across a span or a tile boundary"""
    if codec == V1:
        two = [(i * 37) % 8000 - 4000 for i in range(128)]
        return [("1281-byte literal group", T.VALID["v1 literals/x128 of 10 bytes/i64s"][1:3]), ("257-byte literal group", (E.v1_literals(two, True, [2] * 128), two)),
                ("run of 130", T.VALID["v1 run/x130 step -128 lands on the limit/i64s"][1:3]), ("705-byte literal group", T.VALID["v1 literals/x128 short and long/i64s"][1:3])]
    return [("129-byte literal group", T.VALID["byte literals/x128 of headers/followed"][1:3]), ("byte run of 130", T.VALID["byte run/x130 of 0x00/followed"][1:3])]


@pytest.mark.parametrize("codec", [V1, BYTE])
def test_valid_cases_across_span_and_tile_boundaries(codec):
    """each of the long cases with its header's first byte as the LAST byte of a span (128 KiB), of a tile (512 KiB), and 100 bytes in
    front of either; RLE v1 also 1319, 1320 and 1321 bytes in front of the span boundary: a whole 1281-byte literal group and a few
    bytes.  (They are placements like the others: hop_lds and its LOOK = 1320 in device/rle_scan.hip have no caller, so these three
    meet no edge of LOOK; the short-span walk reads every header from global memory.)"""
    nbits = 64 if codec == V1 else 8
    dtype = TYPES[(codec, nbits)][1]
    places = [(b, k) for b in (SPAN, TILE) for k in (1, 100)] + ([(SPAN, k) for k in (1319, 1320, 1321)] if codec == V1 else [])
    cols, streams, wants = [], [], []
    for boundary, back in places:
        f, fv = to_offset(codec, 0, boundary - back, 1 << 30)
        f, fv = u8(f), np.array(fv, dtype=dtype)
        for name, (stream, want) in straddlers(codec):
            more = (TILE + 4096 - len(fv) - len(want)) // 128 + 1  # (one row count for the stripe: full groups behind the case)
            cols.append(col(len(cols) + 1, codec, nbits))
            streams.append((len(cols), DATA, np.concatenate([f, u8(stream + FULL[codec][0] * more)])))
            wants.append(np.concatenate([fv, np.array(want + FULL[codec][1] * more, dtype=np.int64).astype(dtype)]))
    n = min(len(w) for w in wants)
    assert all(len(w) - n <= 1024 for w in wants)  # (only full groups of the tail are left out)
    for batch in (8192, 1000):
        res = G.gpu_decode(n, cols, streams, batch_size=batch)
        assert res.status()[0] == 0, res.status()
        for ci, c in enumerate(cols):
            assert np.array_equal(values_of(res, ci, codec, nbits), wants[ci][:n]), (ci, batch)
            G.assert_column_parity(res, ci, c, streams, n, batch, what=(ci, batch))
        res.free()


def small_batches(codec, nbits, lo, hi, batch):
    some = [c for c in cases(codec, nbits) if lo <= len(c[2]) <= hi and not c[0].endswith("more in the stream than asked")]
    stream, want = filler(codec, 10)  # the short prefix
    for _name, s, w in some:
        stream, want = stream + s, want + w
    c, s = col(1, codec, nbits), [(1, DATA, u8(stream))]
    res = G.gpu_decode(len(want), [c], s, batch_size=batch)
    check_column(res, 0, c, s, len(want), batch, want, codec, nbits, ("batch", batch, codec, nbits, lo, hi))
    res.free()
    return len(some)


@pytest.mark.parametrize("codec,nbits", CARRIERS)
def test_valid_cases_of_up_to_100_values_at_batch_size_1(codec, nbits):
    """every case of at most 100 values (a batch per value), behind a short prefix: a run's values go out one batch at a time"""
    assert small_batches(codec, nbits, 1, 100, 1) > (60 if codec != V1 else 100)


@pytest.mark.parametrize("codec,nbits", CARRIERS)
def test_valid_long_cases_at_batch_size_7(codec, nbits):
    """the longer cases at a batch size that divides no run"""
    assert small_batches(codec, nbits, 101, 1 << 20, 7) > (50 if codec != V1 else 100)


def test_unsigned_cases():
    """unsigned RLE v1: the LENGTH stream of a Binary column of encoding 0, whose offsets then carry the values"""
    some = [(n, c) for n, c in T.VALID.items() if c[0] == V1 and not c[3] and c[4] == 64 and all(0 <= v <= 1000 for v in c[2])]
    assert len(some) > 150, len(some)
    stream, want = bytearray(), []
    for _name, c in some:
        stream += c[1]
        want += c[2]
    for what, (s, w) in [("one stream", (bytes(stream), want))] + [(n, (c[1], c[2])) for n, c in some[::9]]:
        c = {"column_id": 1, "orc_type": BINARY, "encoding": 0}
        streams = [(1, LENGTH, u8(s)), (1, DATA, np.zeros(max(1, sum(w)), dtype=np.uint8))]
        for batch in (8192, 1000):
            res = G.gpu_decode(len(w), [c], streams, batch_size=batch)
            assert res.status()[0] == 0, (what, res.status())
            lens = np.concatenate([np.diff(res.batch(b, 0)["offsets"]) for b in range(res.n_batches)])
            assert lens.tolist() == w, what
            G.assert_column_parity(res, 0, c, streams, len(w), batch, what=(what, batch))
            res.free()


def test_dictionary_keys_of_encoding_1():
    """a dictionary column of encoding 1: its DATA stream -- the keys -- is hand-built unsigned RLE v1 runs and literals, read by the
    64-bit decoder and stored as 32-bit keys (expand_group<CODEC, 4, 64>); the rows' lengths follow from the keys"""
    words = [("w%d" % i).encode() * (1 + i % 3) for i in range(200)]
    dlens = [len(w) for w in words]
    keys, data = [], b""
    for i in range(300):
        if i % 3 == 0:
            data, keys = data + E.v1_run(i % 60, 1, 3 + i % 128, False), keys + [i % 60 + k for k in range(3 + i % 128)]
        elif i % 3 == 1:
            data, keys = data + E.v1_run(199 - i % 50, -1, 3 + (i * 7) % 128, False, 2 + i % 9), keys + [199 - i % 50 - k for k in range(3 + (i * 7) % 128)]
        else:
            v = [(i * 31 + 7 * k) % 200 for k in range(1 + i % 128)]
            data, keys = data + E.v1_literals(v, False, [1 + (i + k) % 10 if x < 128 else 2 + (i + k) % 9 for k, x in enumerate(v)]), keys + v
    lstream = b"".join(E.v1_literals(dlens[k:k + 128], False) for k in range(0, 200, 128))
    c = {"column_id": 1, "orc_type": STRING, "encoding": 1, "dictionary_size": len(words)}
    streams = [(1, DATA, u8(data)), (1, LENGTH, u8(lstream)), (1, DICT, u8(b"".join(words)))]
    assert E.decode_v1(data, len(keys), False, 64) == keys
    for batch in (8192, 1000):
        res = G.gpu_decode(len(keys), [c], streams, batch_size=batch)
        assert res.status()[0] == 0, res.status()
        lens = np.concatenate([np.diff(res.batch(b, 0)["offsets"]) for b in range(res.n_batches)])
        assert lens.tolist() == [dlens[k] for k in keys], batch
        G.assert_column_parity(res, 0, c, streams, len(keys), batch, what=("dictionary", batch))
        res.free()


# ---- malformed streams: a status word, the oracle's failing batch, every batch in front of it intact -------------------------------
@functools.lru_cache(maxsize=None)
def prefix(codec, offset, long):
    """valid runs that bring the case's header to `offset` of a block: two blocks of them, or (long) to the LAST block of the second
    tile: 2048 blocks, the gate of the exact parallel walk"""
    n0 = len(FULL[codec][0])
    f, fv = to_offset(codec, n0, (2 * TILE - RLE_BLK if long else 2 * RLE_BLK) + offset, 1 << 30)
    return FULL[codec][0] + f, FULL[codec][1] + fv


NO_PREFIX = (b"", [])


def runs_behind(name):
    """for a run that leaves N: valid runs behind it, more than the rows asked -- the stream does not end there, so a decoder that
    misses the overflow delivers values and no status at all (the stream's clean end is OutOfSpec too)"""
    codec, kind = T.MALFORMED[name][0], T.MALFORMED[name][4]
    return FULL[codec][0] * 12 if kind == E.OUT_OF_SPEC and not name.startswith("cut/") else b""


def malformed_cases(codec, nbits, with_front=True):
    names = [n for n, c in T.MALFORMED.items() if (c[0], c[3]) == (codec, nbits) and (c[2] or codec != V1) and (with_front or not n.endswith("/behind valid runs"))]
    return names


def check_malformed(name, front, batch, n_more=T.N_MALFORMED, behind=b"", as_present=False, as_lengths=False):
    """front: (bytes, values) of valid runs in front of the case; behind: bytes of valid runs behind it (what the stream means then:
    the case's run still fails, the table's kind and values hold); as_lengths: an unsigned case as the LENGTH stream of a Binary column"""
    codec, stream, signed, nbits, kind, before = T.MALFORMED[name]
    before = front[1] + before
    n = len(before) + n_more
    if as_lengths:
        assert all(0 <= v <= 1000 for v in before)
        c, s = {"column_id": 1, "orc_type": BINARY, "encoding": 0}, [(1, LENGTH, u8(front[0] + stream + behind)), (1, DATA, np.zeros(max(64, sum(before)), dtype=np.uint8))]
    elif as_present:
        c, s = col(1, V1, 64), [(1, PRESENT, u8(front[0] + stream + behind)), (1, DATA, u8(FULL[V1][0] * (n // 128 + 1)))]
    else:
        c, s = col(1, codec, nbits), [(1, DATA, u8(front[0] + stream + behind))]
    res = G.gpu_decode(n, [c], s, batch_size=batch)
    G.assert_column_parity(res, 0, c, s, n, batch, what=(name, batch))
    st, gbatch, _ = res.status()
    fb = len(before) // batch
    if as_present:
        # array_decoder/mod.rs:228-251: a PRESENT stream that fails is no PRESENT stream: all rows valid from the failing batch on
        assert st == 0, (name, st)
        for b in range(res.n_batches):
            g = res.batch(b, 0)
            bits = [1] * g["length"] if g["validity"] is None else np.unpackbits(np.frombuffer(g["validity"], dtype=np.uint8), bitorder="little")[:g["length"]].tolist()
            assert bits == (before[b * batch:(b + 1) * batch] if b < fb else [1] * g["length"]), (name, batch, b)
    else:
        assert (st, gbatch) == (kind, fb), (name, batch, "gpu", st, gbatch, "table", kind, fb)
        if as_lengths:
            lens = np.concatenate([np.diff(res.batch(b, 0)["offsets"]) for b in range(gbatch)] or [np.zeros(0, np.int32)])
            assert lens.tolist() == before[:fb * batch], (name, batch, "lengths in front of the failing batch")
            res.free()
            return
        dtype = TYPES[(codec, nbits)][1]
        assert np.array_equal(values_of(res, 0, codec, nbits, batches=gbatch), np.array(before[:fb * batch], dtype=np.int64).astype(dtype)), (name, batch, "values in front of the failing batch")
    res.free()


@pytest.mark.parametrize("placement", ["alone", "valid runs behind it"])
@pytest.mark.parametrize("codec,nbits", CARRIERS)
def test_malformed_cases(codec, nbits, placement):
    names = malformed_cases(codec, nbits)
    assert len(names) >= 20, len(names)
    for name in names:
        if placement != "alone" and (T.MALFORMED[name][4] != E.OUT_OF_SPEC or name.startswith("cut/empty")):
            continue  # (valid runs behind a stream that is cut, or behind a varint that goes on, make another stream of it)
        for batch in (8192, 1000):
            check_malformed(name, NO_PREFIX, batch, behind=runs_behind(name) if placement != "alone" else b"")


def family_ends(names):
    """the first and the last member of every family of cases: the names with the base, the count and the byte of a cut left out
    (what stays tells families apart: the error, the kind of run, the step and its sign, the step or the literal that fails, N)"""
    families = {}
    for n in names:
        families.setdefault(re.sub(r"base -?\d+|x\d+|byte \d+( of \d+)?", "#", n), []).append(n)
    return [n for members in families.values() for n in dict.fromkeys((members[0], members[-1]))]


@pytest.mark.parametrize("long", [False, True])
@pytest.mark.parametrize("offset", [0, 1, 510, 511])
@pytest.mark.parametrize("codec,nbits", CARRIERS)
def test_malformed_cases_behind_valid_runs(codec, nbits, offset, long):
    """every case with its header at the four block offsets behind two blocks of valid runs; behind two tiles of them the ends of
    every family of cases (family_ends).  Measured on an MI355X: a call behind two tiles -- a MiB of valid runs, which the oracle
    decodes as well and which is compared batch by batch -- takes 35 ms (booleans, eight rows a byte: 330 ms), every case at both
    batch sizes 9 s for each of the twenty combinations of carrier and offset.  What the two tiles add is the case's place -- the
    last block in front of the gate of the exact walk, across the tile's end --, which every family meets"""
    names = malformed_cases(codec, nbits, with_front=False)
    for name in (family_ends(names) if long else names):
        for batch in (8192, 1000):
            check_malformed(name, prefix(codec, offset, long), batch, behind=runs_behind(name))


@pytest.mark.parametrize("codec,nbits", CARRIERS)
def test_malformed_cases_at_batch_size_1(codec, nbits):
    """every case alone, a batch per value; five values are asked behind the failing run's first"""
    for name in malformed_cases(codec, nbits):
        check_malformed(name, NO_PREFIX, 1, n_more=5)
        if runs_behind(name):
            check_malformed(name, NO_PREFIX, 1, n_more=5, behind=runs_behind(name))


def test_malformed_boolean_cases_as_present_streams():
    for name in malformed_cases(BOOL, 8):
        for batch in (8192, 1000, 1):
            check_malformed(name, NO_PREFIX, batch, n_more=40, as_present=True)
        check_malformed(name, prefix(BOOL, 511, False), 1000, as_present=True)


def test_unsigned_malformed_cases():
    """every unsigned 64-bit case that fails, as the LENGTH stream of a Binary column: the table's kind, the failing batch, the
    lengths in front of it -- alone, with valid runs behind the runs that leave N, and at batch size 1"""
    names = [n for n, c in T.MALFORMED.items() if c[0] == V1 and not c[2] and c[3] == 64]
    assert len(names) >= 100, len(names)
    for name in names:
        for batch in (8192, 1000):
            check_malformed(name, NO_PREFIX, batch, as_lengths=True)
            if runs_behind(name):
                check_malformed(name, NO_PREFIX, batch, behind=runs_behind(name), as_lengths=True)
        check_malformed(name, NO_PREFIX, 1, n_more=5, behind=runs_behind(name), as_lengths=True)


# ---- the walk's paths, and which of them ran --------------------------------------------------------------------------------------
JOB_LINE = re.compile(r"\[orcgpu\] job (\d+) \(stripe \d+ col (\d+) role \d+ block0 \d+ nbits \d+\) codec (\d+) blocks (\d+) group \d+: bad (\d+) \(first (\d+)\) repaired (\d+) total (\d+)")
NONE = 0xFFFFFFFF
CODEC_NUMBER = {V1: 1, BYTE: 2}  # device/rle_parse.h


def walk_calls():
    """(name, codec, [walk stream names]): the columns of one call, the calls in this order"""
    out = []
    for c in (V1, BYTE):
        reg, dec, dense = "regular/" + c, "decoys/" + c, "dense decoys/" + c
        out += [("regular", c, [reg]), ("short", c, ["short/" + c]), ("regular again", c, [reg]), ("changing 1", c, ["changing/" + c]), ("changing 2", c, ["changing/" + c]),
                ("changing 3", c, ["changing/" + c]), ("regular once more", c, [reg]), ("decoys", c, [dec]), ("valid between decoys", c, [dec, reg, dec]),
                ("regular a fourth time", c, [reg]), ("dense decoys 1", c, [dense]), ("dense decoys 2", c, [dense]), ("dense decoys 3", c, [dense]),
                ("regular behind them", c, [reg]), ("dense decoys 4", c, [dense])]
    return out


def cut_byte_streams():
    """two full groups and a third of 1 .. 128 literals (header-like bytes) or a run, cut at every length that leaves its header"""
    out = []
    for count in range(1, 129, 3):
        g = E.byte_literals([(0x05, 0x80, 0xFE, 0x7F)[k % 4] for k in range(count)])
        out += [FULL[BYTE][0] * 2 + g[:cut] for cut in sorted({1, 2, count // 2 + 1, count})]
    return out + [FULL[BYTE][0] * 2 + E.byte_run(9, 20)[:1]]


def child_main():
    """(in the child process, ONE context, the calls in this order: orcgpu_ctx::exact_on is what the call before left) every call's
    columns against the tables' values -- which test_rle1_cases proves to be the model's --; a marker line on stderr in front of
    each call's ORCGPU_DEBUG lines"""
    digests = {}
    for name, codec, columns in walk_calls():
        sys.stderr.write("\nCASE %s/%s\n" % (name, codec))
        sys.stderr.flush()
        built = [T.WALK_STREAMS[w]() for w in columns]
        nbits = built[0][4]
        n = min(len(b[2]) for b in built)
        cols = [col(i + 1, codec, nbits) for i in range(len(built))]
        streams = [(i + 1, DATA, u8(b[1])) for i, b in enumerate(built)]
        res = G.gpu_decode(n, cols, streams)
        ok = res.status()[0] == 0
        for ci, b in enumerate(built):
            got = values_of(res, ci, codec, nbits) if ok else None
            ok = ok and np.array_equal(got, np.array(b[2][:n], dtype=got.dtype))
            digests[(name, codec, ci)] = hash(got.tobytes()) if ok else (name, codec, ci)
        sys.stderr.write("\nRESULT %s/%s %s\n" % (name, codec, "ok" if ok else "WRONG"))
        sys.stderr.flush()
        res.free()
    # byte RLE streams cut inside their last group, a column each: the values the walk counts (the line's `total`) are what
    # test_rle1_cases.walk_total counts -- the stream's last 129 bytes take hop_parse's full parse, which sees the cut
    sys.stderr.write("\nCASE cut byte streams\n")
    sys.stderr.flush()
    cut = cut_byte_streams()
    res = G.gpu_decode(400, [col(i + 1, BYTE, 8) for i in range(len(cut))], [(i + 1, DATA, u8(s)) for i, s in enumerate(cut)])
    sys.stderr.write("\nRESULT cut byte streams %s\n" % ("ok" if res.status()[0] == E.IO_ERROR else "WRONG"))
    res.free()
    same = all(digests[(w + " 1", c, 0)] == digests[(w + " 2", c, 0)] == digests[(w + " 3", c, 0)] for w in ("changing", "dense decoys") for c in (V1, BYTE))
    sys.stderr.write("\nCASE end\nRESULT three-calls-equal %s\n" % ("ok" if same else "WRONG"))


def test_the_walk_paths_and_which_of_them_ran():
    """One child process under ORCGPU_DEBUG; per call and column the library's line `codec C ... bad B (first F) repaired R`: B =
    blocks whose entry was not the exit of the block before when the verify round (rle_walk_kernel mode 2) looked, F = the first of
    them, R = blocks the mending passes (rle_mend_kernel, from RLE_MEND_MIN = 64 bad blocks on) and the serial repair
    (rle_repair_kernel) rewrote.  Every stream has 2048 blocks or more (the gate of the exact parallel walk) and stays under 4 MiB.
    For both codecs: the stride guess (regular), the short-run spans (short, changing, decoys), candidate search and relaxation
    (decoys), the mending passes (decoys), the serial repair -- repair_chain<CODEC_RLE1> and <CODEC_BYTE> -- (changing, dense decoys
    1 and 4), the exact parallel walk -- exact_tables -- (dense decoys 2 and 3, sent because of what the call before left in the
    context).  On the short-run streams only the invariant is asserted -- bad 0 goes with first none and repaired 0."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("ORCGPU_") or k == "ORCGPU_LIB"}  # (the same library in the child)
    env["ORCGPU_DEBUG"] = "1"
    code = "import os, sys; sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests')); import test_gpu_rle1_runs as R; R.child_main()" % (ROOT, ROOT)
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0, err[-3000:]
    calls, results, cur = {}, {}, None
    for line in err.splitlines():
        if line.startswith("CASE "):
            cur = line[5:]
            calls[cur] = {}
        elif line.startswith("RESULT "):
            results[line[7:].rsplit(" ", 1)[0]] = line.rsplit(" ", 1)[1]
        elif cur:
            m = JOB_LINE.search(line)
            if m:
                job, c, codec, blocks, bad, first, repaired, total = (int(x) for x in m.groups())
                calls[cur][c] = dict(codec=codec, blocks=blocks, bad=bad, first=first, repaired=repaired, total=total)
    for name, columns in calls.items():
        for c, d in sorted(columns.items()):
            print("walk %-30s column %d: codec %d  blocks %5d  bad %5d  first %10d  repaired %5d" % (name, c, d["codec"], d["blocks"], d["bad"], d["first"], d["repaired"]))
    assert "end" in calls
    wrong = [k for k, v in results.items() if v != "ok"]
    assert not wrong, ("calls whose values are not the tables'", wrong)
    assert results.get("three-calls-equal") == "ok"
    for name, codec, columns in walk_calls():
        got = calls["%s/%s" % (name, codec)]
        assert len(got) == len(columns), (name, codec, "job lines", got)
        for c, d in got.items():
            assert d["codec"] == CODEC_NUMBER[codec] and d["blocks"] >= 2048, (name, codec, d)
            # the invariants of the three counters (rle_walk_kernel mode 2 counts and records the minimum; repair_chain starts at
            # first_bad, which is inconsistent by definition, and counts every block or run it rewrites)
            if d["bad"] == 0:
                assert d["first"] == NONE and d["repaired"] == 0, (name, codec, d)

    cut = cut_byte_streams()
    totals = calls["cut byte streams"]
    assert len(totals) == len(cut) >= 100, (len(totals), len(cut))
    for i, s in enumerate(cut):
        assert totals[i]["total"] == T.walk_total(s), (i, len(s), totals[i], T.walk_total(s))

    for codec in (V1, BYTE):
        def line(name, c=0):
            got = calls["%s/%s" % (name, codec)]
            return got[sorted(got)[c]]

        # Regular full groups: the stride guess from the first group makes every block strong at its true entry: nothing is inconsistent.
        for name in ("regular", "regular again", "regular once more", "regular a fourth time", "regular behind them"):
            assert line(name)["bad"] == 0, (codec, name, line(name))
        # Groups of ever-changing size whose wrong chains never meet the true one (test_rle1_cases._changing): a span whose
        # warm-up starts at a wrong byte stays wrong, the seam in front of it is inconsistent.  Call 1 comes behind a regular call
        # (exact_on false): the serial repair takes what is left and counts it.  Fewer than RLE_MEND_MIN bad blocks: calls 2 and 3
        # take the same road and report the same.
        first = line("changing 1")
        assert first["bad"] >= 1 and first["first"] < first["blocks"] and first["repaired"] > 0, (codec, first)
        for later in (line("changing 2"), line("changing 3")):
            assert later["bad"] == first["bad"], (codec, first, later)
            if first["bad"] < 64:
                assert later == first, (codec, first, later)
        # Decoys (test_rle1_cases.decoy_stream says why each bites): if the line reports nothing, the decoys did not bite and this
        # test has shown nothing.
        decoys = T.decoy_stream(codec)[2]
        for name, c in (("decoys", 0), ("valid between decoys", 0), ("valid between decoys", 2)):
            d = line(name, c)
            assert d["bad"] >= len(decoys) >= 64 and d["repaired"] >= 1, (codec, name, c, d, len(decoys))
            # (the line is printed behind the mending passes: rle_mend_kernel sets first_bad to none at the stretch it starts from and
            # the verify round behind it, mode 5, records what is left -- none when the passes mended every decoy, as they do here;
            # `bad` is the first verify round's count and stays)
            assert d["first"] == NONE or d["first"] <= decoys[0], (codec, name, c, d)
        # ... and its neighbours' damage does not reach the regular stream between them
        assert line("valid between decoys", 1)["bad"] == 0, (codec, line("valid between decoys", 1))
        # Dense decoys (every second block): an eighth of the blocks and more are bad: rle_hopeless().  Call 1 comes behind a regular
        # call (exact_on false): the serial repair walks the true chain from the first bad block.  Calls 2 and 3 are sent the exact
        # parallel walk: the verify round counts the same blocks, nothing is repaired.  Call 4 comes behind a regular call again.
        dense = T.decoy_stream(codec, 2)[2]
        first = line("dense decoys 1")
        assert len(dense) * 8 >= first["blocks"] and first["bad"] >= len(dense), (codec, first, len(dense))
        assert first["first"] <= dense[0] and first["repaired"] >= first["bad"], (codec, first, dense[0])
        for later in (line("dense decoys 2"), line("dense decoys 3")):
            assert later["bad"] == first["bad"] and later["first"] == NONE and later["repaired"] == 0, (codec, first, later)
        assert line("dense decoys 4") == first, (codec, first, line("dense decoys 4"))
