"""The HIP Decimal128 and Timestamp value decoders on the hand-built tables of tests/test_decimal_cases.py (written with
tests/decimal_enc.py): varints of every encoded length, over-long forms included, placed where varint_terms_body and
varint_decode128_body (device/string_kernels.hip) cut the stream -- at the stream's start, behind 7 bytes, across 8-byte, 64-byte,
2048-byte and 64 KiB boundaries --, malformed streams alone and behind valid filler, the scale repair on its three roads (fused
into the decode, decimal_finish_body behind a PRESENT stream, the uniform flag of rle2_uniform_kernel), and timestamp_body
(device/column_kernels.hip) on the trailing-zero codes, the ORC-763 boundary and the ends of every unit -- against the oracle
(G.assert_column_parity) AND against the plain model's values, bit for bit.

A failing column ends the stripe (one status per result), so every failing case is a call of its own."""
import functools

import numpy as np
import pytest

import decimal_enc as D
import gpu_util as G
import oracle_lib as O
import test_decimal_cases as T
from decimal_enc import M128
from orc_rust_amd import gen

pytestmark = pytest.mark.gpu

DECIMAL, TIMESTAMP = 14, 9
PRESENT, DATA, SECONDARY = 0, 1, 5
MODES = ("uniform", "expanded", "spaced")


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def dcol(cid, scale=0):
    return {"column_id": cid, "orc_type": DECIMAL, "encoding": 2, "precision": 38, "scale": scale}


def i128_bytes(values):
    return b"".join((v & M128).to_bytes(16, "little") for v in values)


def i64_bytes(values):
    return np.array(values, dtype=np.int64).tobytes()


def spaced(values, rows, to_bytes):
    """the values dealt out over the rows of a PRESENT pattern, a zero in every null slot"""
    it = iter(values)
    return to_bytes([next(it) if r else 0 for r in rows])


def row_of(rows, k):
    """the row that holds non-null value k"""
    return k if rows is None else [i for i, r in enumerate(rows) if r][k]


def got_bytes(res, ci, batches=None):
    return b"".join(bytes(res.batch(b, ci)["values"]) for b in range(res.n_batches if batches is None else batches))


def assert_values(got, want, width, what):
    if got != want:
        bad = -1
        if len(got) == len(want):
            a, b = (np.frombuffer(x, dtype=np.uint8).reshape(-1, width) for x in (got, want))
            bad = int(np.nonzero((a != b).any(axis=1))[0][0])
        raise AssertionError((what, "first wrong value", bad, len(got) // width, len(want) // width))


def check_column(res, ci, c, streams, n_rows, batch, want, what, width=16, **kw):
    assert res.status()[0] == 0, (what, res.status())
    assert_values(got_bytes(res, ci), want, width, what)
    G.assert_column_parity(res, ci, c, streams, n_rows, batch, what=what, **kw)


def packed(b, compression):
    return u8(b) if compression == "none" else gen.compress_stream(bytes(b), compression, 64)


def run_valid(cases, mode, batches, compression="none"):
    """cases: [(name, stream, values)] of one value count, a column each, in one call per batch size.
    uniform: a Decimal(38, 0) column whose SECONDARY stream is the constant-0 pattern -- fused, the scales not expanded;
    expanded: one other scale in it -- fused, the scales expanded; spaced: that and a PRESENT stream of 20 % nulls -- the dense
    values go through decimal_finish_body."""
    n = len(cases[0][2])
    assert all(len(v) == n for _, _, v in cases)
    scales = [0] * n
    if mode != "uniform":
        scales[n // 2] = 1
    rows = D.present_rows(n) if mode == "spaced" else None
    n_rows = n if rows is None else len(rows)
    sec = packed(T.constant_scales(0, n) if mode == "uniform" else gen.rle2(np.array(scales, dtype=np.int64), signed=True), compression)
    present = [] if rows is None else [packed(gen.boolean(np.array(rows, dtype=np.uint8)), compression)]
    kw = {} if compression == "none" else {"compression": compression, "block_size": 64}
    cols, streams, wants = [], [], []
    for i, (_name, stream, values) in enumerate(cases):
        cols.append(dcol(i + 1))
        streams += [(i + 1, DATA, packed(stream, compression)), (i + 1, SECONDARY, sec)] + [(i + 1, PRESENT, p) for p in present]
        model = [D.fix_scale(v, 0, s) for v, s in zip(values, scales)]
        wants.append(i128_bytes(model) if rows is None else spaced(model, rows, i128_bytes))
    for batch in batches:
        res = G.gpu_decode(n_rows, cols, streams, batch_size=batch, **kw)
        for ci, c in enumerate(cols):
            check_column(res, ci, c, streams, n_rows, batch, wants[ci], (cases[ci][0], mode, batch, compression), **kw)
        res.free()


def named(prefix):
    return [(name, s, v) for name, (s, v) in T.VALID.items() if name.startswith(prefix)]


# ---- valid varints --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_every_length_at_the_start_and_behind_7_bytes(mode):
    """every single-varint case a column of its own, its varint the stream's first (terminator at p = 0 .. 18: the general path
    below p = 7) and directly behind a 7-byte varint (p = 7 .. 25); at batch sizes 8192, 1000 and 1"""
    cases = named("start/") + named("behind 7 bytes/")
    assert len(cases) == 2 * len(T.VARINTS) >= 2 * 19 * 7
    run_valid(cases, mode, (8192, 1000, 1))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("boundary", [8, 64, 2048])
def test_every_split_across_a_boundary(boundary, mode):
    """every length with every split in front of a thread's 8 bytes, a mask word's 64, a workgroup's 2048: one stream each"""
    run_valid(named("boundary/%d" % boundary), mode, (8192, 1000))


@pytest.mark.parametrize("mode", MODES)
def test_across_one_rank_tile_boundary_and_the_next(mode):
    cases = named("tile/")
    n = min(len(v) for _, _, v in cases)
    assert len(cases) == 7 and all(len(v) - n < 16 for _, _, v in cases)  # (only filler of the tail is left out)
    run_valid([(name, s, v[:n]) for name, s, v in cases], mode, (8192, 1000))


@pytest.mark.parametrize("mode", MODES)
def test_dense_and_sparse_workgroups_and_surplus_values(mode):
    cases = named("density/") + named("surplus/")
    assert len(cases) >= 8
    for case in cases:
        run_valid([case], mode, (8192, 1000))


@pytest.mark.parametrize("compression", ["zlib", "zstd"])
def test_varints_across_chunk_borders(compression):
    """the DATA stream in compression chunks of 64 bytes: varints lie across chunk borders, and the stream's true length is below
    what the call planned for"""
    for name in ("boundary/8", "boundary/64", "density/19-byte varints back to back"):
        for mode in MODES:
            run_valid(named(name), mode, (8192,), compression)


# ---- malformed streams ----------------------------------------------------------------------------------------------------------
PLACEMENTS = {"alone": 0,
              # 16 bytes in front of the boundary: a multiple of 8, so a tail's "length = 0, 1, 7 mod 8" holds as the case was
              # written; the case's own filler (9 .. 16 bytes) then ends at the boundary or just in front of it, and the tail or
              # the long varint lies across it or starts on it
              "behind a workgroup": T.WORKGROUP - 16, "behind a rank tile": T.TILE - 16,
              # 3 bytes in front of the boundary: a malformed varint that is the case's first bytes lies ACROSS the boundary (the
              # tails then end at length = 5, 6, 4 mod 8)
              "across a workgroup boundary": T.WORKGROUP - 3, "across a rank tile boundary": T.TILE - 3}


@functools.lru_cache(maxsize=None)
def front(placement):
    return D.fill_bytes(PLACEMENTS[placement])


def check_failing_decimal(what, data, sec, n_values, rows, batch, kind, index, before, scale=0):
    """value `index` fails with `kind`: the status word, the batch of the row that holds the value, every batch in front intact"""
    n_rows = n_values if rows is None else len(rows)
    c = dcol(1, scale)
    streams = [(1, DATA, u8(data)), (1, SECONDARY, u8(sec))] + ([] if rows is None else [(1, PRESENT, gen.boolean(np.array(rows, dtype=np.uint8)))])
    res = G.gpu_decode(n_rows, [c], streams, batch_size=batch)
    st, gbatch, _ = res.status()
    failing = row_of(rows, index) // batch
    assert (st, gbatch) == (kind, failing), (what, "gpu", st, gbatch, "model", kind, failing)
    have = failing * batch  # rows of the batches in front
    if rows is None:
        want = i128_bytes(before[:have])
    else:
        assert sum(rows[:have]) <= len(before)
        want = spaced(before[:sum(rows[:have])], rows[:have], i128_bytes)
    assert_values(got_bytes(res, 0, batches=failing), want, 16, (what, "values in front of the failing batch"))
    G.assert_column_parity(res, 0, c, streams, n_rows, batch, what=what)
    res.free()


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("placement", list(PLACEMENTS))
def test_malformed_streams(placement, nulls):
    fbytes, fvals = front(placement)
    for name, (stream, n, kind, index, before) in T.MALFORMED.items():
        n_values = len(fvals) + n
        rows = D.present_rows(n_values) if nulls else None
        batches = (1000, 8192) if "rank tile" in placement else (1000, 4) if n <= 200 else (1000,)
        for batch in batches:
            check_failing_decimal((name, placement, nulls, batch), fbytes + stream, T.constant_scales(0, n_values), n_values, rows, batch,
                                  kind, len(fvals) + index, fvals + before)


def test_both_streams_of_a_column_short():
    for name, (data, sec, n_rows, batch, (kind, failing)) in T.BOTH_SHORT.items():
        model = D.decode(data, n_rows)
        assert isinstance(model, tuple)
        # (DATA's own failing value for the front; the failing batch is the case's: SECONDARY may fail first)
        c = dcol(1, T.BOTH_SCALE)
        streams = [(1, DATA, u8(data)), (1, SECONDARY, u8(sec))]
        res = G.gpu_decode(n_rows, [c], streams, batch_size=batch)
        assert res.status()[:2] == (kind, failing), (name, res.status(), kind, failing)
        assert_values(got_bytes(res, 0, batches=failing), i128_bytes(model[2][:failing * batch]), 16, (name, "values in front of the failing batch"))
        G.assert_column_parity(res, 0, c, streams, n_rows, batch, what=name)
        res.free()


# ---- scale repair ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("road", ["fused", "spaced"])
@pytest.mark.parametrize("f", T.COLUMN_SCALES)
def test_scale_grid(f, road):
    cells = [(s, v, w) for cf, s, v, w in T.GRID if cf == f]
    assert len(cells) >= 50
    model = [D.fix_scale(v, f, s) for s, v, _ in cells]
    assert model == [w for _, _, w in cells]
    rows = D.present_rows(len(cells)) if road == "spaced" else None
    n_rows = len(cells) if rows is None else len(rows)
    c = dcol(1, f)
    streams = [(1, DATA, u8(b"".join(D.varint(v) for _, v, _ in cells))), (1, SECONDARY, gen.rle2(np.array([s for s, _, _ in cells], dtype=np.int64), signed=True))]
    if rows is not None:
        streams.append((1, PRESENT, gen.boolean(np.array(rows, dtype=np.uint8))))
    want = i128_bytes(model) if rows is None else spaced(model, rows, i128_bytes)
    for batch in (8192, 100):
        res = G.gpu_decode(n_rows, [c], streams, batch_size=batch)
        check_column(res, 0, c, streams, n_rows, batch, want, ("scale grid", f, road, batch))
        res.free()


@pytest.mark.parametrize("f", T.COLUMN_SCALES)
def test_scales_that_are_the_columns_scale_over_the_edge_values(f):
    """the uniform road (rle2_uniform_kernel sets the flag, the scales are never expanded): the values go through as they are"""
    values = T.EDGE_VALUES * 30  # (more than two runs of 512)
    c = dcol(1, f)
    streams = [(1, DATA, u8(b"".join(D.varint(v) for v in values))), (1, SECONDARY, u8(T.constant_scales(f, len(values))))]
    for batch in (8192, 1000):
        res = G.gpu_decode(len(values), [c], streams, batch_size=batch)
        check_column(res, 0, c, streams, len(values), batch, i128_bytes(values), ("uniform scales", f, batch))
        res.free()


@pytest.mark.parametrize("road", ["fused", "spaced"])
def test_where_the_reference_panics(road):
    """a wrapped power of ten that is 0: the reference panics, oracle and HIP path leave the value as it is.
    Oracle parity only -- the model says PANICS and nothing else."""
    for f in T.COLUMN_SCALES:
        cells = [(s, v) for cf, s, v in T.PANICS if cf == f]
        assert len(cells) >= 4 and all(D.fix_scale(v, f, s) == D.PANICS for s, v in cells)
        rows = D.present_rows(len(cells)) if road == "spaced" else None
        n_rows = len(cells) if rows is None else len(rows)
        c = dcol(1, f)
        streams = [(1, DATA, u8(b"".join(D.varint(v) for _, v in cells))), (1, SECONDARY, gen.rle2(np.array([s for s, _ in cells], dtype=np.int64), signed=True))]
        if rows is not None:
            streams.append((1, PRESENT, gen.boolean(np.array(rows, dtype=np.uint8))))
        res = G.gpu_decode(n_rows, [c], streams)
        assert res.status()[0] == 0, (f, road, res.status())
        G.assert_column_parity(res, 0, c, streams, n_rows, 8192, what=("panics", f, road))
        res.free()


# ---- timestamps -----------------------------------------------------------------------------------------------------------------
UNITS = (D.SECONDS, D.MILLIS, D.MICROS, D.NANOS)
MUST_FAIL = {D.SECONDS: ["-1 s, 1 ns code 0", "0 s, 999999999 ns code 0"], D.MILLIS: ["-1 s, 1 ns code 0", "0 s, 999999 ns code 0"],
             D.MICROS: ["-1 s, 1 ns code 0", "0 s, 1 ns code 1"],
             D.NANOS: ["9223372037 s, 0 ns code 0", "-9223372037 s, 0 ns code 0", "9223372036 s, 854775808 ns code 0", "-9223372036 s, 145224191 ns code 0"]}


def tcol(unit):
    if unit == D.DECIMAL128:
        return {"column_id": 1, "orc_type": TIMESTAMP, "encoding": 2, "arrow_target": 20, "arrow_precision": 38, "arrow_scale": 9}
    return {"column_id": 1, "orc_type": TIMESTAMP, "encoding": 2, "arrow_target": unit + 1}


def ts_streams(table, rows):
    s = [(1, DATA, gen.rle2(np.array([r[1] for r in table], dtype=np.int64), signed=True)),
         (1, SECONDARY, gen.rle2(np.array([r[2] for r in table], dtype=np.int64), signed=False))]
    return s + ([] if rows is None else [(1, PRESENT, gen.boolean(np.array(rows, dtype=np.uint8)))])


@functools.lru_cache(maxsize=None)
def good_rows(unit, at_least=2600):
    """the rows the unit takes, over and over: several batches of them"""
    ok = [r for r in T.TS_ROWS if unit == D.DECIMAL128 or r[3][unit] != D.DECODE_TIMESTAMP]
    assert len(ok) >= 20, (unit, len(ok))
    return ok * (at_least // len(ok) + 1)


def ts_want(table, unit, rows):
    model = [D.decode_timestamp(T.TS_BASE, r[1], r[2], unit) for r in table]
    assert model == [r[3][unit] for r in table]
    to_bytes = i128_bytes if unit == D.DECIMAL128 else i64_bytes
    return to_bytes(model) if rows is None else spaced(model, rows, to_bytes)


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("unit", UNITS + (D.DECIMAL128,))
def test_timestamp_rows(unit, nulls):
    """every row of the table that the unit takes: the trailing-zero codes, nanoseconds of 10^9 and more, the wrapping multiply,
    ORC-763 at 999 999 and 1 000 000 ns, the ends of i64 nanoseconds.  The Decimal128(38, 9) target takes every row; the oracle has
    no such column, the model judges it alone."""
    table = good_rows(unit)
    rows = D.present_rows(len(table)) if nulls else None
    n_rows = len(table) if rows is None else len(rows)
    c, streams = tcol(unit), ts_streams(table, rows)
    want = ts_want(table, unit, rows)
    for batch in (8192, 1000):
        res = G.gpu_decode(n_rows, [c], streams, batch_size=batch)
        assert res.status()[0] == 0, (unit, nulls, batch, res.status())
        assert_values(got_bytes(res, 0), want, 16 if unit == D.DECIMAL128 else 8, ("timestamp rows", unit, nulls, batch))
        if unit != D.DECIMAL128:
            G.assert_column_parity(res, 0, c, streams, n_rows, batch, ts_unit=unit, ts_base=T.TS_BASE, what=("timestamp rows", unit, nulls, batch))
        res.free()


def check_failing_timestamps(what, unit, table, bad_at, nulls, batch):
    """bad_at: the (non-null) rows of `table` that fail; the first of them names the batch, every batch in front is intact"""
    rows = D.present_rows(len(table)) if nulls else None
    n_rows = len(table) if rows is None else len(rows)
    c, streams = tcol(unit), ts_streams(table, rows)
    res = G.gpu_decode(n_rows, [c], streams, batch_size=batch)
    failing = row_of(rows, min(bad_at)) // batch
    assert res.status()[:2] == (O.DECODE_TIMESTAMP, failing), (what, res.status(), failing)
    have = failing * batch
    good = [r[3][unit] for r in table[:min(bad_at)]]
    want = i64_bytes(good[:have]) if rows is None else spaced(good[:sum(rows[:have])], rows[:have], i64_bytes)
    assert_values(got_bytes(res, 0, batches=failing), want, 8, (what, "values in front of the failing batch"))
    G.assert_column_parity(res, 0, c, streams, n_rows, batch, ts_unit=unit, ts_base=T.TS_BASE, what=what)
    res.free()


def failing_rows(unit):
    """EVERY row of the table that the unit refuses"""
    return [r for r in T.TS_ROWS if r[3][unit] == D.DECODE_TIMESTAMP]


def must_fail(unit):
    must = [r for r in failing_rows(unit) if r[0] in MUST_FAIL[unit]]
    assert len(must) == len(MUST_FAIL[unit]) >= 2, (unit, [r[0] for r in must])
    return must


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("unit", UNITS)
def test_every_timestamp_row_that_fails(unit, nulls):
    """every row of the table the unit refuses -- loss of precision and overflow, under every trailing-zero code -- in a call of
    its own: 40 good rows around it, batches of 16, the failing row in the second or third of them"""
    good, bad = good_rows(unit)[:40], failing_rows(unit)
    assert len(bad) >= 100 and len(bad) + len({r[0] for r in good_rows(unit)}) == len(T.TS_ROWS), (unit, len(bad))
    for i, row in enumerate(bad):
        at = 17 + i % 16
        check_failing_timestamps((row[0], unit, nulls), unit, good[:at] + [row] + good[at:], [at], nulls, 16)


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("unit", UNITS)
def test_timestamp_rows_that_fail_behind_many_good_rows(unit, nulls):
    """the plainest failures (1 ns asked as microseconds, a second and a nanosecond beyond i64 nanoseconds, ...) in a column of
    2600 rows and more, at batch sizes 8192 and 1000: the failing row in the second batch of 1000"""
    table = list(good_rows(unit))
    for i, row in enumerate(must_fail(unit)):
        at = 1700 + 7 * i
        for batch in (8192, 1000):
            check_failing_timestamps((row[0], unit, nulls, batch), unit, table[:at] + [row] + table[at:], [at], nulls, batch)


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("unit", UNITS)
def test_the_first_failing_timestamp_row_wins(unit, nulls):
    table, bad = list(good_rows(unit, 4200)), must_fail(unit)
    # two failing rows in different batches: the first one's batch is reported
    two = table[:1200] + [bad[0]] + table[1200:3400] + [bad[-1]] + table[3400:]
    check_failing_timestamps(("two failing rows", unit, nulls), unit, two, [1200, 3401], nulls, 1000)
    # the first failing row behind three full batches: those are intact
    check_failing_timestamps(("behind three batches", unit, nulls), unit, table[:3017] + [bad[1]] + table[3017:], [3017], nulls, 1000)
