"""Hand-built Decimal128 DATA streams, scale repairs and Timestamp rows (tests/decimal_enc.py), judged without a GPU by the plain
model and by the CPU oracle.

The tables, built once at import and shared with tests/test_gpu_decimal_cases.py:
  VARINTS     name -> (bytes, value)                one varint; the value follows from the payload the case was written from
  VALID       name -> (stream, values)              a DATA stream and the values a column asks of it (the stream may hold more)
  MALFORMED   name -> (stream, n, kind, index, values in front)   n values are asked; value `index` fails with `kind`
  BOTH_SHORT  name -> (DATA, SECONDARY, rows, batch, (kind, failing batch))   a column both of whose streams run dry
  GRID        [(column scale, value scale, value, value at the column's scale)]
  PANICS      [(column scale, value scale, value)]  the reference divides by a wrapped power of ten that is 0
  TS_ROWS     [(name, DATA value, SECONDARY value, {unit: value or DECODE_TIMESTAMP})]
Every expected value is worked out here, next to the case, from the fields the case was written from -- not by the model.  Model
and oracle must agree with it on every case; the model alone must pass the reference's own decimal vectors (tests/kat_vectors.py).

Stream offsets that matter to the HIP decoder (device/string_kernels.hip: varint_terms_body, varint_decode128_body): a thread
owns 8 stream bytes, a terminator mask word 64, a workgroup (and its LDS stage) 2048, a rank tile 64 KiB; a terminator at stream
offset p < 7 cannot take the two-word fast path, and no varint of 8 bytes or more can."""
import random
import zlib

import decimal_enc as D
import kat_vectors as K
import oracle_lib as O
import rle2_enc as R
from decimal_enc import I128_MAX, I128_MIN, M128

VARINTS, VALID, MALFORMED, BOTH_SHORT = {}, {}, {}, {}
GRID, PANICS, TS_ROWS = [], [], []
LENGTHS = range(1, 20)
WORD, MASK_WORD, WORKGROUP, TILE = 8, 64, 2048, 65536
N_START = 40  # values of a "start" / "behind 7 bytes" stream
TS_BASE = 1_420_070_400


def rnd(name):
    return random.Random(zlib.crc32(name.encode()))


def from_u(u):
    """the value a zigzag payload stands for: an even payload is twice a non-negative value, an odd one 2 |v| - 1 of a negative"""
    return u // 2 if u % 2 == 0 else -(u + 1) // 2


def wrap128(v):
    v &= M128
    return v - (1 << 128) if v >> 127 else v


def bytes_of(u, nbytes):
    b = D.raw(D.groups_of(u))
    assert len(b) == nbytes, (u, nbytes, len(b))
    return b


def one(name, data, value):
    assert name not in VARINTS, name
    VARINTS[name] = (bytes(data), value)


def valid(name, stream, values):
    assert name not in VALID, name
    VALID[name] = (bytes(stream), list(values))


def malformed(name, stream, n, kind, index, front):
    assert name not in MALFORMED and index < n, name
    MALFORMED[name] = (bytes(stream), n, kind, index, list(front))


# ---- single varints: every encoded length ---------------------------------------------------------------------------------------
for L in LENGTHS:
    lo, hi = (0 if L == 1 else 1 << 7 * (L - 1)), min((1 << 7 * L) - 1, M128)
    # (of a 19-byte varint only 128 of the 133 payload bits exist: its largest payloads are i128::MAX and i128::MIN)
    for kind, u in (("smallest +", lo), ("smallest -", lo + 1), ("largest +", hi - 1), ("largest -", hi)):
        one("%d bytes/%s" % (L, kind), bytes_of(u, L), from_u(u))
    # over-long forms: continuation bytes that carry nothing
    for what, v in (("zero", 0), ("+1", 1), ("-1", -1)):
        one("%d bytes/%s padded" % (L, what), D.varint(v, L), v)
assert VARINTS["19 bytes/largest +"][1] == I128_MAX and VARINTS["19 bytes/largest -"][1] == I128_MIN
# the 19th byte sits at offset 126: its bits 2 .. 6 lie above bit 127 and fall off
G18 = [0x2A + i for i in range(18)]
LOW126 = sum(g << 7 * i for i, g in enumerate(G18))
one("19 bytes/19th byte all ones", D.raw(G18 + [0x7F]), from_u(LOW126 | 3 << 126))
one("19 bytes/19th byte only bits above 127", D.raw(G18 + [0x7C]), from_u(LOW126))
one("19 bytes/19th byte bit 127 and above", D.raw(G18 + [0x7E]), from_u(LOW126 | 1 << 127))
one("19 bytes/nothing but a bit above 127", D.raw([0] * 18 + [0x04]), 0)
one("19 bytes/odd payload, bits above 127", D.raw([1] + [0] * 17 + [0x78]), -1)


def payload(L, name):
    """a varint of L bytes whose every group carries bits (seeded by its name): (bytes, value)"""
    u = (rnd(name).getrandbits(7 * L) | 1 << 7 * (L - 1) | 1 << min(7 * L - 1, 126)) & M128
    return bytes_of(u, L), from_u(u)


# ---- placements -----------------------------------------------------------------------------------------------------------------
SEVEN, SEVEN_VALUE = bytes_of(6 * 10**12, 7), 3 * 10**12
for name, (data, value) in list(VARINTS.items()):
    # at the very start of a stream: the terminator at p = L - 1; p < 7 takes the general path whatever the length
    f, fv = D.fill1(N_START - 1)
    valid("start/" + name, data + f, [value] + fv)
    # directly behind a 7-byte varint: the terminator at p = 7 .. 25
    f, fv = D.fill1(N_START - 2)
    valid("behind 7 bytes/" + name, SEVEN + data + f, [SEVEN_VALUE, value] + fv)
SPLITS = [(L, s) for L in LENGTHS for s in range(1, L)]


def boundary_stream(B):
    """every length with every split: s bytes of the varint in front of a multiple of B, the rest behind it; fillers between"""
    out, vals = bytearray(), []
    for L, s in SPLITS:
        f, fv = D.fill_bytes((-s - len(out)) % B, at=len(vals))
        data, value = payload(L, "boundary %d/%d/%d" % (B, L, s))
        out += f + data
        vals += fv + [value]
        assert (len(out) - L + s) % B == 0
    f, fv = D.fill_bytes(B + 3, at=len(vals))
    return bytes(out) + f, vals + fv


for B in (WORD, MASK_WORD, WORKGROUP):
    valid("boundary/%d" % B, *boundary_stream(B))
# across a rank-tile boundary and across the next one (trank of a tile's first word comes from the tile sums)
TILE_SPLITS = sorted({(L, s) for L in (2, 7, 8, 19) for s in (1, L - 1)})
for L, s in TILE_SPLITS:
    out, vals = bytearray(), []
    for k in (1, 2):
        f, fv = D.fill_bytes(k * TILE - s - len(out), at=len(vals))
        data, value = payload(L, "tile %d/%d/%d" % (k, L, s))
        out += f + data
        vals += fv + [value]
    f, fv = D.fill_bytes(WORKGROUP + 5, at=len(vals))
    valid("tile/%d bytes, %d in front" % (L, s), bytes(out) + f, vals + fv)

# ---- density --------------------------------------------------------------------------------------------------------------------
valid("density/2048 one-byte varints", *D.fill1(2048))  # a workgroup's bytes all terminators: the LDS stage full
valid("density/2049 one-byte varints", *D.fill1(2049))
packed = [payload(19, "packed %d" % i) for i in range(216)]  # 4104 bytes: the fewest terminators valid varints allow, two workgroups
valid("density/19-byte varints back to back", b"".join(p[0] for p in packed), [p[1] for p in packed])
# more values than the rows need: the surplus is not looked at, whatever it holds
f, fv = D.fill1(3000)
valid("surplus/500 values", f, fv[:2500])
valid("surplus/one value", f, fv[:2999])
f, fv = D.fill_bytes(5003)
valid("surplus/an unterminated tail", f + b"\x80" * 5, fv)
valid("surplus/a 25-byte varint", f + D.varint(7, 25) + D.fill1(9)[0], fv)
valid("surplus/a 25-byte varint behind the workgroup", f[:2048] + D.fill1(2048)[0] + D.varint(7, 25), fv[:256] + D.fill1(1000)[1])

# ---- malformed streams ----------------------------------------------------------------------------------------------------------
for L in (20, 21, 25):  # byte 20 of a varint is read and then refused (offset 133 >= 128)
    long = D.varint(12345, L)
    malformed("%d bytes/value 0" % L, long + D.fill1(30)[0], 20, D.VARINT_TOO_LARGE, 0, [])
    f, fv = D.fill_bytes(107)
    malformed("%d bytes/mid-stream" % L, f + long + D.fill1(30)[0], len(fv) + 10, D.VARINT_TOO_LARGE, len(fv), fv)
    malformed("%d bytes/the last value needed" % L, f + long + D.fill1(30)[0], len(fv) + 1, D.VARINT_TOO_LARGE, len(fv), fv)
for what, byte in (("0x80", b"\x80"), ("0xff", b"\xff")):  # a workgroup (and more) without a terminator, valid values behind
    malformed("3000 continuation bytes %s/value 0" % what, byte * 3000 + b"\x01" + D.fill1(50)[0], 20, D.VARINT_TOO_LARGE, 0, [])
    f, fv = D.fill1(5)
    malformed("3000 continuation bytes %s/value 5" % what, f + byte * 3000 + b"\x01" + D.fill1(50)[0], 20, D.VARINT_TOO_LARGE, 5, fv)
for t in list(range(1, 20)) + [20, 40]:  # the stream ends inside a varint: 19 bytes can still be read, the 20th is refused
    for r in (0, 1, 7):
        k = next(k for k in range(9, 17) if (k + t) % 8 == r)
        f, fv = D.fill1(k, at=t)
        malformed("tail of %d bytes/length = %d mod 8" % (t, r), f + (b"\xff" if t & 1 else b"\x80") * t, k + 3,
                  D.IO_ERROR if t <= 19 else D.VARINT_TOO_LARGE, k, fv)
N_CLEAN = 12
for what, last in (("short", -300), ("long", -(10**30))):  # 2 and 15 bytes: fast path, general path
    last, value = D.varint(last), [last]
    assert len(last) in (2, 15)
    malformed("clean end/1 of %d values, the last one %s" % (N_CLEAN, what), last, N_CLEAN, D.IO_ERROR, 1, value)
    f, fv = D.fill1(N_CLEAN - 2)
    malformed("clean end/%d of %d values, the last one %s" % (N_CLEAN - 1, N_CLEAN, what), f + last, N_CLEAN, D.IO_ERROR, N_CLEAN - 1, fv + value)
malformed("clean end/0 of %d values" % N_CLEAN, b"", N_CLEAN, D.IO_ERROR, 0, [])
malformed("empty stream/1 value asked", b"", 1, D.IO_ERROR, 0, [])
malformed("empty stream/5000 values asked", b"", 5000, D.IO_ERROR, 0, [])


# ---- both streams of a column short ---------------------------------------------------------------------------------------------
def constant_scales(scale, n):
    """a SECONDARY stream as every writer makes it: DELTA runs of 512 with a fixed delta of 0, and a shorter last one"""
    return b"".join(R.delta(scale, 0, 0, [], min(512, n - at), True) for at in range(0, n, 512))


BOTH_ROWS, BOTH_BATCH, BOTH_SCALE = 5000, 1000, 2
for what, kd, ks in (("DATA runs dry in an earlier batch", 1500, 3500), ("DATA runs dry in a later batch", 3500, 1500),
                     ("the same batch, DATA shorter", 2300, 2700), ("the same batch, SECONDARY shorter", 2700, 2300)):
    # a batch reads its varints first, then its scales (array_decoder/decimal.rs:129-130): in the batch both fail, DATA's error is
    # the one; a SECONDARY stream that ends where a run begins is OutOfSpec (rle_v2/mod.rs:115-123)
    bd, bs = kd // BOTH_BATCH, ks // BOTH_BATCH
    BOTH_SHORT[what] = (D.fill8(kd)[0], constant_scales(BOTH_SCALE, ks), BOTH_ROWS, BOTH_BATCH, (O.IO_ERROR, bd) if bd <= bs else (O.OUT_OF_SPEC, bs))

# ---- scale repair ---------------------------------------------------------------------------------------------------------------
COLUMN_SCALES = (0, 1, 2, 18, 37, 38)
EDGE_VALUES = [0, 1, -1, I128_MIN, I128_MAX, I128_MAX // 10 + 1, -(I128_MAX // 10) - 1, (1 << 64) + 12345, -(1 << 100) - 7, 3 * 10**37 + 9, 12345678901234567890123456789]
for k in (1, 2, 18, 19, 37, 38):
    EDGE_VALUES += [s * (10**k + d) for s in (1, -1) for d in (-1, 0, 1)]
EDGE_VALUES = sorted(set(EDGE_VALUES))


def value_scales(f):
    return sorted({s for s in (f, f + 1, f - 1, 0, 38, 39, f + 38, f + 39, f + 127) if s >= 0})


def at_scale(v, f, s):
    """v of scale s >= 0 at scale f: divided by 10^(s - f) as 128 bits hold it, toward zero; or multiplied, in 128 bits"""
    if s <= f:
        return wrap128(v * 10 ** (f - s))  # (f <= 38: the power itself never wraps)
    d = wrap128(10 ** (s - f))  # from 10^39 on this is not the power any more; it is never 0 below 10^128
    q = v // d
    return wrap128(q + 1 if q < 0 and q * d != v else q)  # floor -> truncation


for f in COLUMN_SCALES:
    for s in value_scales(f):
        for v in EDGE_VALUES:
            GRID.append((f, s, v, at_scale(v, f, s)))
for f in COLUMN_SCALES:
    for s in (f + 128, 2**31 - 1, -1, -(2**31)):
        for v in (0, 1, -1, 10**20, I128_MIN):
            PANICS.append((f, s, v))

# ---- timestamps -----------------------------------------------------------------------------------------------------------------
# i64 nanoseconds end at 9223372036.854775807 s and begin at -9223372036.854775808 s, which ORC writes as second -9223372036 with
# 145224192 ns: below the epoch and more than 999 999 ns, so a second is taken off (ORC-763) -- -9223372037 s + 0.145224192 s
TS_PAYLOADS = (0, 1, 999_999, 1_000_000, 999_999_999, 10**9, 5 * 10**9 + 3, 184_467_440_738, 854_775_807, 854_775_808, 145_224_192, 145_224_191)
TS_SECONDS = (-1, 0, -TS_BASE, 9_223_372_036, -9_223_372_036, 9_223_372_037, -9_223_372_037)  # seconds since the UNIX epoch
assert 184_467_440_738 * 10**8 >= 1 << 64  # code 7 wraps the u64 multiply


def ts_want(sse, pay, code):
    nn = pay * 10 ** (code + 1) % (1 << 64) if code else pay  # code 0 means "as it is", code z "z + 1 zeros were cut"
    ns = (sse - 1 if sse < 0 and nn >= 1_000_000 else sse) * 10**9 + nn
    want = {D.DECIMAL128: ns}
    for unit, per in enumerate(D.NANOS_PER_UNIT):
        want[unit] = ns // per if ns % per == 0 and D.I64_MIN <= ns // per <= D.I64_MAX else D.DECODE_TIMESTAMP
    return want


for sse in TS_SECONDS:
    for code in range(8):
        for pay in TS_PAYLOADS:
            TS_ROWS.append(("%d s, %d ns code %d" % (sse, pay, code), sse - TS_BASE, pay << 3 | code, ts_want(sse, pay, code)))


# ---- the tests ------------------------------------------------------------------------------------------------------------------
def test_the_tables_have_the_cases():
    print("decimal cases: %d varints, %d valid streams, %d malformed, %d scale cells, %d panics, %d timestamp rows"
          % (len(VARINTS), len(VALID), len(MALFORMED), len(GRID), len(PANICS), len(TS_ROWS)))
    for L in LENGTHS:
        assert sum(1 for n, (b, _) in VARINTS.items() if len(b) == L and ("smallest" in n or "largest" in n)) >= 4, L
        assert sum(1 for b, _ in VARINTS.values() if len(b) == L) >= 7, L
        assert "start/%d bytes/largest -" % L in VALID and "behind 7 bytes/%d bytes/zero padded" % L in VALID
    assert len(SPLITS) >= 170 and all(("boundary/%d" % B) in VALID for B in (8, 64, 2048))
    assert len(TILE_SPLITS) == 7 and sum(n.startswith("tile/") for n in VALID) == 7
    assert len(MALFORMED) >= 60 and len(BOTH_SHORT) >= 3
    assert len(GRID) >= 300 and len(PANICS) >= 4 * len(COLUMN_SCALES)
    assert {s - f for f, s, _v, _w in GRID} >= {0, 1, -1, 38, 39, 127}
    assert len(TS_ROWS) >= 8 * 7 * 7
    for unit in range(4):  # every unit has rows it takes and rows it refuses
        kinds = {r[3][unit] == D.DECODE_TIMESTAMP for r in TS_ROWS}
        assert kinds == {True, False}, unit
    for name, (stream, values) in VALID.items():
        assert len(stream) < 1 << 20 and len(values) < 300_000, name


def test_the_constant_scales_are_the_pattern_the_uniform_road_looks_for():
    """rle2_uniform_kernel (device/rle_expand.hip) sets its flag only for C1 FF zz 00 over and over -- DELTA, fixed delta 0, 512
    values of zigzag zz -- and a shorter last run of the same kind: what the GPU file's "uniform" mode relies on"""
    for f in COLUMN_SCALES + (BOTH_SCALE,):
        for n in (1, 2, 40, 511, 512, 513, 1024, 1500, 44524):
            s, full, rest = constant_scales(f, n), n // 512, n % 512
            assert s[:4 * full] == bytes([0xC1, 0xFF, 2 * f, 0x00]) * full, (f, n)
            assert s[4 * full:] == (bytes([0xC0 | (rest - 1) >> 8, (rest - 1) & 0xFF, 2 * f, 0x00]) if rest else b""), (f, n)
            assert R.decode(s, n, True, 32) == [f] * n


def test_the_boundary_streams_place_what_they_say():
    """s bytes in front of the boundary, L - s behind it, for every case of the three boundary streams and the tile streams"""
    for B in (WORD, MASK_WORD, WORKGROUP):
        stream, values = VALID["boundary/%d" % B]
        pos, seen = 0, set()
        for _ in values:
            n = 1 + next(i for i in range(19) if not stream[pos + i] & 0x80)
            seen |= {(n, s) for s in range(1, n) if (pos + s) % B == 0}
            pos += n
        assert pos == len(stream)
        assert set(SPLITS) <= seen, (B, sorted(set(SPLITS) - seen)[:5])
    for L, s in TILE_SPLITS:
        stream, _ = VALID["tile/%d bytes, %d in front" % (L, s)]
        for k in (1, 2):
            head = stream[k * TILE - s:k * TILE - s + L]
            assert not head[-1] & 0x80 and all(b & 0x80 for b in head[:-1]) and not stream[k * TILE - s - 1] & 0x80, (L, s, k)


def test_the_writer_writes_the_shortest_form_and_the_references_vectors():
    for name, (data, value) in VARINTS.items():
        if "smallest" in name or "largest" in name:
            assert D.varint(value) == data, name
    for name, data, want in K.VARINT_I128:
        assert b"".join(D.varint(v) for v in want) == bytes(data), name


def test_model_passes_the_references_vectors():
    assert len(K.VARINT_I128) >= 2
    for name, data, want in K.VARINT_I128:
        assert D.decode(bytes(data), len(want)) == list(want), name
        assert D.decode(bytes(data), len(want) + 1) == (D.IO_ERROR, len(want), list(want)), name
    # encoding/decimal.rs:93-108 and :110-138: skip all, then EOF
    assert D.decode(bytes([0x14, 0x28]), 3) == (D.IO_ERROR, 2, [10, 20])


def test_model_and_oracle_agree_on_every_single_varint():
    wrong = []
    for name, (data, value) in VARINTS.items():
        got, (st, ovals) = D.decode(data, 1), O.varint128(data, 1)
        if got != [value] or st != O.OK or ovals != [value]:
            wrong.append((name, got, st, ovals, value))
        # ... and one byte less is the end of the stream inside a varint (or an empty stream)
        if D.decode(data[:-1], 1) != (D.IO_ERROR, 0, []) or O.varint128(data[:-1], 1)[0] != O.IO_ERROR:
            wrong.append((name, "a byte short"))
    assert not wrong, (len(wrong), wrong[:10])


def test_model_and_oracle_agree_on_every_valid_stream():
    wrong = []
    for name, (stream, want) in VALID.items():
        got = D.decode(stream, len(want))
        st, ovals = O.varint128(stream, len(want))
        if got != want or st != O.OK or ovals != want:
            bad = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), -1) if isinstance(got, list) else got[:2]
            wrong.append((name, "model: first wrong value", bad, "oracle", st, ovals == want))
    assert not wrong, (len(wrong), wrong[:10])


def test_model_and_oracle_agree_on_every_malformed_stream():
    wrong = []
    for name, (stream, n, kind, index, front) in MALFORMED.items():
        got = D.decode(stream, n)
        st, _ = O.varint128(stream, n)
        if got != (kind, index, front) or st != kind:
            wrong.append((name, "model", got[:2] if isinstance(got, tuple) else "values", "oracle", st, "want", kind, index))
            continue
        # the values in front of the failing one are there: the oracle has exactly those, and not one more
        st, ovals = O.varint128(stream, index)
        if st != O.OK or ovals != front or O.varint128(stream, index + 1)[0] != kind:
            wrong.append((name, "values in front of the failing one", index, st))
    assert not wrong, (len(wrong), wrong[:10])


def decimal_column(data, secondary, precision=38, scale=0, present=None):
    streams = {1: bytes(data), 5: bytes(secondary)}
    if present is not None:
        streams[0] = bytes(present)
    return O.Column(14, 2, streams, precision=precision, scale=scale)


def test_model_and_oracle_column_agree_on_the_boundary_streams():
    """the oracle's column decoder (varints, then scales, batch by batch) over the three boundary streams at two batch sizes"""
    for B in (WORD, MASK_WORD, WORKGROUP):
        stream, want = VALID["boundary/%d" % B]
        model = D.decode(stream, len(want))
        assert model == want
        for batch in (8192, 1000):
            c = decimal_column(stream, constant_scales(0, len(want)))
            assert c.status == O.OK
            for at in range(0, len(want), batch):
                n = min(batch, len(want) - at)
                b = c.next_batch(n)
                assert b["status"] == O.OK, (B, batch, at)
                assert b["values"] == b"".join((v & M128).to_bytes(16, "little") for v in model[at:at + n]), (B, batch, at)
            c.close()


def test_both_streams_short_fail_as_the_text_says():
    for name, (data, secondary, rows, batch, (kind, failing)) in BOTH_SHORT.items():
        c = decimal_column(data, secondary, scale=BOTH_SCALE)
        assert c.status == O.OK
        model = D.decode(data, rows)
        for b in range(rows // batch):
            got = c.next_batch(batch)
            if b < failing:
                # (the DATA values are of the column's scale: they go through unchanged)
                front = model[2] if isinstance(model, tuple) else model
                assert got["status"] == O.OK and got["values"] == b"".join((v & M128).to_bytes(16, "little") for v in front[b * batch:(b + 1) * batch]), (name, b)
            else:
                assert (got["status"], b) == (kind, failing), (name, got["status"], b)
                break
        c.close()
    # the same batch: whichever stream is shorter, the varints are read first
    assert BOTH_SHORT["the same batch, DATA shorter"][4] == BOTH_SHORT["the same batch, SECONDARY shorter"][4] == (O.IO_ERROR, 2)


def test_model_and_oracle_agree_on_the_scale_grid():
    wrong = []
    for f, s, v, want in GRID:
        got, ogot = D.fix_scale(v, f, s), O.fix_scale(v, f, s)
        if got != want or ogot != want:
            wrong.append((f, s, v, "want", want, "model", got, "oracle", ogot))
    assert not wrong, (len(wrong), wrong[:5])
    # the grid does wrap: powers of ten from 10^39 on, and products
    assert sum(1 for f, s, v, w in GRID if s - f >= 39 and w != 0) >= 20
    assert sum(1 for f, s, v, w in GRID if s < f and w != v * 10 ** (f - s)) >= 20


def test_where_the_reference_panics():
    """PANICS holds the divisor-0 cells and nothing else; the model says PANICS for exactly these; the oracle leaves the value"""
    for f, s, v in PANICS:
        k = (s & 0xFFFFFFFF) - f
        assert k >= 128 and pow(10, k, 1 << 128) == 0, (f, s)
        assert D.fix_scale(v, f, s) == D.PANICS, (f, s, v)
        assert O.fix_scale(v, f, s) == v, (f, s, v)
    assert {s - f for f, s, _ in PANICS} >= {128} and {s for _, s, _ in PANICS} >= {2**31 - 1, -1, -(2**31)}
    assert not any(D.fix_scale(v, f, s) == D.PANICS for f, s, v, _ in GRID)
    assert D.fix_scale(5, 0, 127) == 0 and D.fix_scale(5, 0, 128) == D.PANICS  # the last power that is not 0, and the first that is


def test_model_and_oracle_agree_on_every_timestamp_row():
    wrong = []
    for name, secs, nanos, want in TS_ROWS:
        for unit in range(4):
            got = D.decode_timestamp(TS_BASE, secs, nanos, unit)
            st, oval = O.decode_timestamp(TS_BASE, secs, nanos, unit)
            ogot = oval if st == O.OK else st
            assert st in (O.OK, O.DECODE_TIMESTAMP)
            if got != want[unit] or (ogot != want[unit] if st == O.OK else want[unit] != D.DECODE_TIMESTAMP):
                wrong.append((name, unit, "want", want[unit], "model", got, "oracle", st, oval))
        if D.decode_timestamp(TS_BASE, secs, nanos, D.DECIMAL128) != want[D.DECIMAL128]:
            wrong.append((name, "decimal128"))
    assert not wrong, (len(wrong), wrong[:5])


def test_the_timestamp_rows_hold_the_edges():
    rows = {r[0]: r[3] for r in TS_ROWS}
    assert rows["9223372036 s, 854775807 ns code 0"][D.NANOS] == D.I64_MAX
    assert rows["9223372036 s, 854775808 ns code 0"][D.NANOS] == D.DECODE_TIMESTAMP
    assert rows["-9223372036 s, 145224192 ns code 0"][D.NANOS] == D.I64_MIN
    assert rows["-9223372036 s, 145224191 ns code 0"][D.NANOS] == D.DECODE_TIMESTAMP
    assert rows["9223372037 s, 0 ns code 0"] == {0: 9223372037, 1: 9223372037000, 2: 9223372037000000, 3: D.DECODE_TIMESTAMP, 4: 9223372037 * 10**9}
    # ORC-763: at 999 999 ns the second stays, at 1 000 000 ns it is taken off -- below the epoch only
    assert rows["-1 s, 999999 ns code 0"][D.NANOS] == -(10**9) + 999_999 and rows["-1 s, 1000000 ns code 0"][D.NANOS] == -2 * 10**9 + 10**6
    assert rows["0 s, 1000000 ns code 0"][D.NANOS] == 10**6
    assert rows["-1 s, 1 ns code 0"][D.MICROS] == D.DECODE_TIMESTAMP and rows["-1 s, 1 ns code 2"][D.MICROS] == -(10**6) + 1
    # 10^9 ns and more are taken as they are; the u64 multiply wraps under code 7
    assert rows["0 s, 1000000000 ns code 0"][D.SECONDS] == 1
    assert rows["0 s, 184467440738 ns code 7"][D.DECIMAL128] == 184_467_440_738 * 10**8 - (1 << 64)
