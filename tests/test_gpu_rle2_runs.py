"""The HIP integer RLE v2 decoder on the hand-built runs of tests/test_rle2_cases.py (written with tests/rle2_enc.py): forms no
encoder of this project emits, placed where the scan pass (device/rle_scan.hip) cuts the stream -- at block offsets 0, 1, 510 and
511 of a 512-byte block, across block, span (256 blocks) and tile (1024 blocks) boundaries, alone, behind valid runs and in front
of them, at batch sizes 8192, 1000 and 1 -- against the oracle (G.assert_column_parity) AND against the plain model's values.
Then the walk's paths, and which of them ran: a child process under ORCGPU_DEBUG whose per-job lines are read.

Signed cases are the DATA stream of a Long / Int / Short column (N = i64 / i32 / i16); unsigned ones the LENGTH stream of a Binary
column, as in test_gpu_kat.py -- those whose values can be lengths (0 .. 1000); the others are judged off the GPU only.
A failing column ends the stripe (one status per result), so every malformed case is a call of its own."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gpu_util as G
import rle2_enc as E
import test_rle2_cases as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RLE_BLK, SPAN, TILE = 512, 256 * 512, 1024 * 512
TYPES = {64: (4, np.int64), 32: (3, np.int32), 16: (2, np.int16)}  # Long, Int, Short
BINARY, DATA, LENGTH = 8, 1, 2
FULL_VALUES = [(i * 5) % 200 - 100 for i in range(512)]
FULL = E.direct(FULL_VALUES, 7, True)  # a full run: DIRECT, 8 bits, 512 values, 514 bytes


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def col(cid, nbits):
    return {"column_id": cid, "orc_type": TYPES[nbits][0], "encoding": 2}


def values_of(res, ci, dtype, batches=None):
    return np.concatenate([np.frombuffer(res.batch(b, ci)["values"], dtype=dtype) for b in range(res.n_batches if batches is None else batches)] or [np.zeros(0, dtype)])


def filler(k):
    """valid runs of exactly k bytes (k >= 3): full runs, then one DIRECT run of 8-bit values that takes the rest"""
    out, vals = b"", []
    while k > 517:
        out, vals, k = out + FULL, vals + FULL_VALUES, k - len(FULL)
    if k > 514:
        out, vals, k = out + E.direct(FULL_VALUES[:100], 7, True), vals + FULL_VALUES[:100], k - 102
    return out + E.direct(FULL_VALUES[:k - 2], 7, True), vals + FULL_VALUES[:k - 2]


def to_offset(at, offset, modulus=RLE_BLK):
    """filler that brings a stream of `at` bytes to `offset` modulo `modulus`"""
    k = (offset - at) % modulus
    return filler(k if k >= 3 else k + modulus) if k else (b"", [])


def signed_cases(nbits):
    return [(name, c) for name, c in T.VALID.items() if c[2] and c[3] == nbits]


def one_stream(cases, offset):
    """every case's first byte at block offset `offset`, fillers between them and a full run behind the last"""
    out, vals = bytearray(FULL), list(FULL_VALUES)
    for _name, (stream, want, _s, _n) in cases:
        f, fv = to_offset(len(out), offset)
        out += f + stream
        vals += fv + want
    while len(out) < 2049 * RLE_BLK:  # 2048 blocks and more: the call passes the gate of the exact parallel walk
        out, vals = out + FULL, vals + FULL_VALUES
    return bytes(out), vals


def check_column(res, ci, c, streams, n, batch, want, dtype, what):
    assert res.status()[0] == 0, (what, res.status())
    got = values_of(res, ci, dtype)
    if got.tolist() != want:
        bad = next(i for i, (a, b) in enumerate(zip(got.tolist(), want)) if a != b) if len(got) == len(want) else -1
        raise AssertionError((what, "first wrong value", bad, len(got), len(want)))
    G.assert_column_parity(res, ci, c, streams, n, batch, what=what)


@pytest.mark.parametrize("nbits", T.NBITS)
def test_valid_cases_alone(nbits):
    """every case a column of its own (its run is the stream's first and last), all in one call"""
    cases = signed_cases(nbits)
    for part in range(0, len(cases), 600):
        chunk = cases[part:part + 600]
        n = max(len(c[1]) for _, c in chunk)
        # (a column has the stripe's row count: shorter cases get full runs behind them -- the suffix placement)
        cols, streams, wants = [], [], []
        for i, (name, (stream, want, _s, _n)) in enumerate(chunk):
            pad_runs = (n - len(want) + 511) // 512
            cols.append(col(i + 1, nbits))
            streams.append((i + 1, DATA, u8(stream + FULL * pad_runs)))
            wants.append((want + FULL_VALUES * pad_runs)[:n])
        for batch in (8192, 1000):
            res = G.gpu_decode(n, cols, streams, batch_size=batch)
            for ci, c in enumerate(cols):
                check_column(res, ci, c, streams, n, batch, wants[ci], TYPES[nbits][1], (chunk[ci][0], batch))
            res.free()


@pytest.mark.parametrize("offset", [0, 1, 510, 511])
@pytest.mark.parametrize("nbits", T.NBITS)
def test_valid_cases_in_one_stream_at_block_offsets(nbits, offset):
    """all cases of one N in ONE stream (1 - 2 MiB: thousands of blocks, several spans and tiles), each case's header at the same
    offset of a block: the runs' payloads lie across block boundaries all over, every case has valid runs in front and behind"""
    stream, want = one_stream(signed_cases(nbits), offset)
    assert 2048 * RLE_BLK < len(stream) < 4 << 20, len(stream)
    c, s = col(1, nbits), [(1, DATA, u8(stream))]
    for batch in (8192, 1000):
        res = G.gpu_decode(len(want), [c], s, batch_size=batch)
        check_column(res, 0, c, s, len(want), batch, want, TYPES[nbits][1], (nbits, offset, batch))
        res.free()


def straddlers(nbits):
    """one long case (or more) of every sub-encoding: their payloads are what can lie across a span or a tile boundary"""
    names = ["direct/w%d/n512" % nbits, "direct/w7/n511", "direct/w1/n512", "patched/list: 31 entries", "patched/list: two fillers",
             "patched/patch 11 + gap 2 = 13 bits", "delta packed/w64/n20/first -7", "delta packed/w3/n20/first +0", "delta fixed/n512/step -1",
             "short_repeat/%d bytes/x10" % (nbits // 8), "mixed/PATCHED then DELTA/long"]
    return [(n, T.VALID["%s/i%ds" % (n, nbits)]) for n in names]


@pytest.mark.parametrize("nbits", T.NBITS)
def test_valid_cases_across_span_and_tile_boundaries(nbits):
    """each of the long cases with its header's first byte as the LAST byte of a span (128 KiB), of a tile (512 KiB), and 100 bytes in
    front of either: the header itself, and then the payload, lie across the boundary"""
    dtype = TYPES[nbits][1]
    cols, streams, wants = [], [], []
    for boundary in (SPAN, TILE):
        for back in (1, 100):
            f, fv = to_offset(0, boundary - back, 1 << 30)
            f, fv = u8(f), np.array(fv, dtype=dtype)
            for name, (stream, want, _s, _n) in straddlers(nbits):
                more = (TILE - len(fv)) // 512 + 3  # (one row count for the stripe: full runs behind the case)
                cols.append(col(len(cols) + 1, nbits))
                streams.append((len(cols), DATA, np.concatenate([f, u8(stream + FULL * more)])))
                wants.append(np.concatenate([fv, np.array(want + FULL_VALUES * more, dtype=dtype)]))
    n = min(len(w) for w in wants)
    assert all(len(w) - n <= 1024 + 512 for w in wants)  # (only full runs of the tail are left out)
    for batch in (8192, 1000):
        res = G.gpu_decode(n, cols, streams, batch_size=batch)
        assert res.status()[0] == 0, res.status()
        for ci, c in enumerate(cols):
            assert np.array_equal(values_of(res, ci, dtype), wants[ci][:n]), (ci, batch)
            G.assert_column_parity(res, ci, c, streams, n, batch, what=(ci, batch))
        res.free()


def small_batches(nbits, lo, hi, batch):
    cases = [(n, c) for n, c in signed_cases(nbits) if lo <= len(c[1]) <= hi]
    stream, want = E.direct(FULL_VALUES[:9], 7, True), FULL_VALUES[:9]  # the short prefix
    for _name, (s, w, _s, _n) in cases:
        stream, want = stream + s, want + w
    c, s = col(1, nbits), [(1, DATA, u8(stream))]
    res = G.gpu_decode(len(want), [c], s, batch_size=batch)
    check_column(res, 0, c, s, len(want), batch, want, TYPES[nbits][1], ("batch", batch, nbits, lo, hi))
    res.free()
    return len(cases)


@pytest.mark.parametrize("nbits", T.NBITS)
def test_valid_cases_of_up_to_10_values_at_batch_size_1(nbits):
    """EVERY short case (a batch per value), behind a short prefix: a run's values go out one batch at a time"""
    assert small_batches(nbits, 1, 10, 1) > 300


@pytest.mark.parametrize("nbits", T.NBITS)
def test_valid_cases_of_up_to_100_values_at_batch_size_1(nbits):
    """... and every case of 11 to 100 values: all the patch width x gap width cases (12 values), DELTA runs of 20, DIRECT runs of 63 - 65"""
    assert small_batches(nbits, 11, 100, 1) > 300


@pytest.mark.parametrize("nbits", T.NBITS)
def test_valid_long_cases_at_batch_size_7(nbits):
    """the cases of more than 100 values (the patch lists, runs of 511 and 512, the long pairs) at a batch size that divides no run: at
    batch size 1 they would be 50 000 batches and more a column, read one by one"""
    assert small_batches(nbits, 101, 1 << 20, 7) > 50


def test_unsigned_cases():
    """unsigned RLE v2: the LENGTH stream of a Binary column, whose offsets then carry the values"""
    cases = [(n, c) for n, c in T.VALID.items() if not c[2] and c[3] == 64 and all(0 <= v <= 1000 for v in c[1])]
    assert len(cases) > 150, len(cases)
    stream, want = bytearray(), []
    for _name, (s, w, _s, _n) in cases:
        stream += s
        want += w
    for what, (s, w) in [("one stream", (bytes(stream), want))] + [(n, (c[0], c[1])) for n, c in cases[::9]]:
        c = {"column_id": 1, "orc_type": BINARY, "encoding": 2}
        streams = [(1, LENGTH, u8(s)), (1, DATA, np.zeros(max(1, sum(w)), dtype=np.uint8))]
        for batch in (8192, 1000):
            res = G.gpu_decode(len(w), [c], streams, batch_size=batch)
            assert res.status()[0] == 0, (what, res.status())
            lens = np.concatenate([np.diff(res.batch(b, 0)["offsets"]) for b in range(res.n_batches)])
            assert lens.tolist() == w, what
            G.assert_column_parity(res, 0, c, streams, len(w), batch, what=(what, batch))
            res.free()


# ---- malformed streams: a status word, the oracle's failing batch, every batch in front of it intact -------------------------------
@functools.lru_cache(maxsize=None)
def prefix(offset, long):
    """valid runs that bring the case's header to `offset` of a block: two blocks of them, or (long) to the LAST block of the second
    tile: 2048 blocks, the gate of the exact parallel walk; the case lies behind seven span boundaries and a tile boundary, and from
    offset 510 or 511 its run lies across the end of the tile"""
    f, fv = to_offset(len(FULL), (2 * TILE - RLE_BLK if long else 0) + offset, 1 << 30 if long else RLE_BLK)
    return u8(FULL + f), np.array(FULL_VALUES + fv, dtype=np.int64)


NO_PREFIX = (u8(b""), np.zeros(0, dtype=np.int64))


def check_malformed(name, stream, front, signed, nbits, batch, n_more=T.N_MALFORMED + 3 * 512):
    """front: (bytes, values) of valid runs in front of the case; the model judges the case alone (its failing run and the values in
    front of it move by what stands in front)"""
    model = E.decode(stream, T.N_MALFORMED + 3 * 512, signed, nbits)
    fails = isinstance(model, tuple)
    dtype = TYPES[nbits][1]
    before = np.concatenate([front[1].astype(dtype), np.array(model[2] if fails else model, dtype=np.int64).astype(dtype)])
    n = len(before) + n_more if fails else len(before)
    if signed:
        c, s = col(1, nbits), [(1, DATA, np.concatenate([front[0], u8(stream)]))]
    else:  # the LENGTH stream of a Binary column
        c, s = {"column_id": 1, "orc_type": BINARY, "encoding": 2}, [(1, LENGTH, u8(stream)), (1, DATA, np.zeros(64, dtype=np.uint8))]
    res = G.gpu_decode(n, [c], s, batch_size=batch)
    G.assert_column_parity(res, 0, c, s, n, batch, what=(name, batch))
    if not signed:
        assert res.status()[0] != 0, (name, "a status word")
    elif fails and model[0] != E.PANICS:
        st, gbatch, _ = res.status()
        assert (st, gbatch) == (model[0], len(before) // batch), (name, batch, "gpu", st, gbatch, "model", model[0], len(before) // batch)
        assert np.array_equal(values_of(res, 0, dtype, batches=gbatch), before[:gbatch * batch]), (name, batch, "values in front of the failing batch")
    elif not fails:
        assert res.status()[0] == 0 and np.array_equal(values_of(res, 0, dtype), before), (name, batch)
    res.free()


def malformed_cases(signed=True):
    return [(name, case[:3]) for table in (T.MALFORMED, T.PANICS) for name, case in table.items() if case[1] == signed]


@pytest.mark.parametrize("placement", ["alone", "valid runs behind it"])
def test_malformed_cases(placement):
    for name, (stream, signed, nbits) in malformed_cases():
        for batch in (8192, 1000):
            # (valid runs behind it: whatever the stream means then -- the model and the oracle say)
            check_malformed((name, placement), stream + (FULL * 3 if placement != "alone" else b""), NO_PREFIX, signed, nbits, batch)


@pytest.mark.parametrize("long", [False, True])
@pytest.mark.parametrize("offset", [0, 1, 510, 511])
def test_malformed_cases_behind_valid_runs(offset, long):
    """every case with its header at the four block offsets, behind two blocks of valid runs and behind a tile of them (the header
    at offset 511 of the tile's last block: the run lies across the tile boundary)"""
    for name, (stream, signed, nbits) in malformed_cases():
        for batch in ((8192,) if long else (8192, 1000)):
            check_malformed((name, offset, long), stream, prefix(offset, long), signed, nbits, batch)


def test_malformed_cases_at_batch_size_1():
    """every case alone, a batch per value; five values are asked behind the failing run's first"""
    for name, (stream, signed, nbits) in malformed_cases():
        check_malformed((name, "batch 1"), stream, NO_PREFIX, signed, nbits, 1, n_more=5)


def test_unsigned_malformed_cases():
    """unsigned streams that fail, as the LENGTH stream of a Binary column: a status word, and the oracle's batch and kind"""
    cases = malformed_cases(signed=False)
    assert len(cases) >= 20, len(cases)
    for name, (stream, signed, nbits) in cases:
        if nbits == 64:  # (a LENGTH stream is unsigned 64-bit whatever the column; the narrow cases are for the model and the oracle)
            for batch in (8192, 1000):
                check_malformed((name, "unsigned"), stream, NO_PREFIX, False, 64, batch)


# ---- the walk's paths, and which of them ran --------------------------------------------------------------------------------------
JOB_LINE = re.compile(r"\[orcgpu\] job (\d+) \(stripe \d+ col (\d+) role \d+ block0 \d+ nbits \d+\) codec \d+ blocks (\d+) group \d+: bad (\d+) \(first (\d+)\) repaired (\d+) total (\d+)")
NONE = 0xFFFFFFFF
CARRIER = 513  # bytes of a decoy stream's run: DIRECT, 8 bits, 511 values


@functools.lru_cache(maxsize=None)
def regular_stream(runs=2200):
    vals = [(i * 37) % 60000 - 30000 for i in range(512)]
    return E.direct(vals, 15, True) * runs, vals * runs  # 16-bit values: 1026 bytes a run


def short_stream(runs=260000):
    out, vals = bytearray(), []
    for i in range(runs):
        if i % 3 == 0:
            out += E.short_repeat(i % 100 - 50, 3 + i % 8, 1, True)
            vals += [i % 100 - 50] * (3 + i % 8)
        else:
            v = [(i + k * 7) % 120 - 60 for k in range(1 + i % 8)]
            out += E.direct(v, 7, True)
            vals += v
    return bytes(out), vals


def flush_stream(runs=2300):
    out, vals = bytearray(), []
    for i in range(runs):
        v = FULL_VALUES if i % 20 != 19 else FULL_VALUES[:272]  # 10 000 rows a row group: 19 full runs and one of 272
        out += E.direct(v, 7, True)
        vals += v
    return bytes(out), vals


@functools.lru_cache(maxsize=None)
def changing_stream(size=2200 * 1024):
    out, vals, i = bytearray(), [], 0
    while len(out) < size:
        n = 200 + (i * i * 7 + i * 13) % 312  # 200 .. 511 values of 64 bits: no full run, no stride
        v = [((i + 1) * (k + 3) * 0x9E3779B97F4A7C15) % (1 << 64) - (1 << 63) for k in range(n)]
        out += E.direct(v, 31, True)
        vals += v
        i += 1
    return bytes(out), vals


@functools.lru_cache(maxsize=None)
def decoy_stream(every=8, runs=2300):
    """A SHORT_REPEAT run (no stride to guess from: every block searches), then runs of 511 8-bit values (513 bytes: no block has a
    full-run header of its own, every block is weak).  In every `every`-th run whose successor's header lies at block offset
    300 .. 500 the payload spells DIRECT / 1 bit / 512 values (0x41 0xff: 66 bytes) at block offsets o, o + 66, o + 132 and o + 198
    of the successor's block, o = 10 + (decoy number mod 4): the search's first candidate there, and three more of its kind follow
    at its size -- plausible_header() passes, the block is strong at entry o, while the true chain enters it at 300 .. 500.
    Why every decoy bites (rle_walk_kernel mode 1): the block in front of a decoy block is weak, so the decoy block keeps its entry
    unless the chain from that block's exit arrives exactly at o.  The true chain's exit is 300 and more: behind o.  A false chain
    -- the one a decoy block sends on -- hops through the payload's 0x10 bytes (SHORT_REPEAT of three bytes: 4 bytes a hop), so it
    keeps its position modulo 4 (66 x 4 and 512 are multiples of 4): it joins the true chain at the first header of the same
    residue (a header's residue grows by one per run: within four runs), and it can arrive at a later decoy's o only if that o has
    the residue of the decoy it came from -- which the `mod 4` above rules out for the next three decoys; by the fourth it has
    long joined the true chain.  Returns (stream, values, blocks with a decoy)."""
    out, decoys = bytearray(E.short_repeat(1, 3, 1, True)), []
    words = [1, 1, 1]
    for k in range(runs):
        payload = [0x10] * 511
        nxt = len(out) + CARRIER  # the next run's header
        if 300 <= nxt % RLE_BLK <= 500 and k % every == 0 and k + 1 < runs:
            b0 = nxt - nxt % RLE_BLK
            for o in (10, 76, 142, 208):
                i = b0 + o + len(decoys) % 4 - (len(out) + 2)
                payload[i], payload[i + 1] = 0x41, 0xFF
            decoys.append(b0 // RLE_BLK)
        out += E.direct(payload, 7, False)
        words += payload
    vals = [1, 1, 1] + [(u >> 1) ^ -(u & 1) for u in words[3:]]
    return bytes(out), vals, decoys


def walk_calls():
    """name -> [(stream, values)] : the columns of one call"""
    decoy, dense = decoy_stream()[:2], decoy_stream(every=2)[:2]
    return [("regular", [regular_stream()]), ("short", [short_stream()]), ("flush", [flush_stream()]), ("regular again", [regular_stream()]),
            ("changing 1", [changing_stream()]), ("changing 2", [changing_stream()]), ("changing 3", [changing_stream()]),
            ("regular once more", [regular_stream()]), ("decoys", [decoy]), ("valid between decoys", [decoy, regular_stream(), decoy]),
            ("regular a fourth time", [regular_stream()]), ("dense decoys 1", [dense]), ("dense decoys 2", [dense]), ("dense decoys 3", [dense]),
            ("regular behind them", [regular_stream()]), ("dense decoys 4", [dense])]


def child_main():
    """(in the child process, ONE context, the calls in this order: orcgpu_ctx::exact_on is what the call before left) every call's
    columns against the model; a marker line on stderr in front of each call's ORCGPU_DEBUG lines"""
    digests, models = {}, {}
    for name, columns in walk_calls():
        sys.stderr.write("\nCASE %s\n" % name)
        sys.stderr.flush()
        n = min(len(v) for _, v in columns)
        cols = [col(i + 1, 64) for i in range(len(columns))]
        streams = [(i + 1, DATA, u8(s)) for i, (s, _) in enumerate(columns)]
        res = G.gpu_decode(n, cols, streams)
        ok = res.status()[0] == 0
        for ci, (s, v) in enumerate(columns):
            if s not in models:
                models[s] = E.decode(s, len(v), True, 64)
            model = models[s][:n]
            got = values_of(res, ci, np.int64).tolist() if ok else None
            ok = ok and model == v[:n] and got == model
            digests[(name, ci)] = hash(tuple(got or ()))
        sys.stderr.write("\nRESULT %s %s\n" % (name, "ok" if ok else "WRONG"))
        sys.stderr.flush()
        res.free()
    same = all(digests[(w + " 1", 0)] == digests[(w + " 2", 0)] == digests[(w + " 3", 0)] for w in ("changing", "dense decoys"))
    sys.stderr.write("\nCASE end\nRESULT three-calls-equal %s\n" % ("ok" if same else "WRONG"))


def test_the_walk_paths_and_which_of_them_ran():
    """One child process under ORCGPU_DEBUG; per call and column the library's line `bad B (first F) repaired R`: B = blocks whose entry
    was not the exit of the block before when the verify round (rle_walk_kernel mode 2) looked, F = the first of them, R = blocks the
    mending passes (rle_mend_kernel, only from RLE_MEND_MIN = 64 bad blocks on) and the serial repair (rle_repair_kernel) rewrote.
    Every stream has 2048 blocks or more (the gate of the exact parallel walk) and stays under 4 MiB.  Reached: the stride guess
    (regular), the short-run spans (short, changing, decoys), candidate search, fill and relaxation (flush, decoys), the mending
    passes (decoys), the serial repair (changing, dense decoys 1 and 4), the exact parallel walk (dense decoys 2 and 3, sent
    because of what the call before left in the context).  On the short-run and the row-group streams only the invariant is
    asserted -- bad 0 goes with first none and repaired 0 --, their counts are printed: how many warm-ups miss the true chain is
    the heuristics' business."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("ORCGPU_")}
    env["ORCGPU_DEBUG"] = "1"
    code = "import os, sys; sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests')); import test_gpu_rle2_runs as R; R.child_main()" % (ROOT, ROOT)
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
                job, c, blocks, bad, first, repaired, total = (int(x) for x in m.groups())
                calls[cur][c] = dict(blocks=blocks, bad=bad, first=first, repaired=repaired, total=total)
    for name, columns in calls.items():
        for c, d in sorted(columns.items()):
            print("walk %-22s column %d: blocks %5d  bad %5d  first %10d  repaired %5d" % (name, c, d["blocks"], d["bad"], d["first"], d["repaired"]))
    assert "end" in calls
    wrong = [k for k, v in results.items() if v != "ok"]
    assert not wrong, ("calls whose values are not the model's", wrong)
    assert results.get("three-calls-equal") == "ok"
    n_cols = {name: len(c) for name, c in walk_calls()}
    for name, want in n_cols.items():
        assert len(calls[name]) == want, (name, "job lines", calls[name])
        for c, d in calls[name].items():
            assert d["blocks"] >= 2048, (name, d)
            # the invariants of the three counters (rle_walk_kernel mode 2 counts and records the minimum; repair_chain starts at
            # first_bad, which is inconsistent by definition, and counts every block or run it rewrites)
            if d["bad"] == 0:
                assert d["first"] == NONE and d["repaired"] == 0, (name, d)

    def line(name, c=0):
        return calls[name][sorted(calls[name])[c]]

    # Regular full runs: the stride guess from the first run (mode 0; DIRECT: "self sized", its two header bytes at gp - s0 and gp
    # equal the stream's first two) makes every block strong at its true entry or pass-through: nothing is inconsistent.
    for name in ("regular", "regular again", "regular once more", "regular a fourth time", "regular behind them"):
        assert line(name)["bad"] == 0, (name, line(name))
    # Runs of ever-changing size: no header names 512 values, so no candidate verifies and every block is weak; the short-run spans
    # are exact inside a span, but a warm-up of 32 blocks (16 KiB = 5 - 10 runs) started at a wrong byte need not meet the true chain.
    # Call 1 comes behind a regular call (exact_on false): whatever is left goes to the serial repair, which counts it.
    # It must report repaired blocks.  With fewer than RLE_MEND_MIN = 64 bad blocks (printed above) rle_mend_kernel returns at once,
    # bad_left is never written and exact_on stays false: calls 2 and 3 then take the same road and report the same.
    first = line("changing 1")
    assert first["bad"] >= 1 and first["first"] < first["blocks"] and first["repaired"] > 0, first
    for later in (line("changing 2"), line("changing 3")):
        assert later["bad"] == first["bad"], (first, later)
        if first["bad"] < 64:
            assert later == first, (first, later)
    # Decoys: every block searches (the stride guess fails on the SHORT_REPEAT run in front), the decoy is its block's first
    # candidate and passes plausible_header(); the block before is weak, so the relaxation rounds let the strong block keep its
    # entry (mode 1: `keep = true`; pex = 300 .. 500 is not below e = 10).  The verify round must find it: entry 10, exit of the
    # block before 300 .. 500.  If it reports nothing, the decoy did not bite and this test has shown nothing.
    decoys = decoy_stream()[2]
    for name, c in (("decoys", 0), ("valid between decoys", 0), ("valid between decoys", 2)):
        d = line(name, c)
        # every decoy bites (decoy_stream's docstring), the first bad block is no later than the first decoy's, and 64 bad blocks
        # and more make the mending passes run; what they and the serial repair rewrite is at least one block
        assert d["bad"] >= len(decoys) >= 64 and d["repaired"] >= 1, (name, c, d, len(decoys))
        assert d["first"] == NONE or d["first"] <= decoys[0], (name, c, d)
    # ... and its neighbours' damage does not reach the regular stream between them
    assert line("valid between decoys", 1)["bad"] == 0, line("valid between decoys", 1)
    # Dense decoys (a decoy in every second block of a window: every decoy bites, so an eighth of the stream's blocks and more are
    # bad): rle_hopeless().  Call 1 comes behind a regular call (exact_on false): rle_mend_kernel does nothing but set bad_left = bad,
    # the mode-5 verify returns, the exact kernels are not sent, and the serial repair walks the true chain from the first bad
    # block: it counts every run or block it rewrites, at least one per bad block.  bad_left >= RLE_EXACT_MIN sets exact_on.
    dense = decoy_stream(every=2)[2]
    first = line("dense decoys 1")
    assert len(dense) * 8 >= first["blocks"] and first["bad"] >= len(dense), (first, len(dense))
    assert first["first"] <= dense[0] and first["repaired"] >= first["bad"], (first, dense[0])
    # Calls 2 and 3 are sent the exact parallel walk: the verify round counts the same blocks, the mending passes still do
    # nothing (hopeless), rle_exact_chain_kernel clears first_bad and rle_repair_kernel returns at once: nothing is counted.
    for later in (line("dense decoys 2"), line("dense decoys 3")):
        assert later["bad"] == first["bad"] and later["first"] == NONE and later["repaired"] == 0, (first, later)
    # Call 4 comes behind a regular call again (which cleared exact_on): the serial repair, as in call 1 -- the road a stream
    # takes depends on the call before it, the values do not (RESULT lines: all four equal the model's).
    assert line("dense decoys 4") == first, (first, line("dense decoys 4"))
