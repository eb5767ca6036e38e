"""Hand-built integer RLE v2 runs (tests/rle2_enc.py), judged without a GPU by the plain model and by the CPU oracle.

Three tables, built once at import and shared with tests/test_gpu_rle2_runs.py:
  VALID      name -> (stream, values, signed, nbits)   the values follow from the header fields the case was written from,
                                                       worked out here next to the case, not by the model
  MALFORMED  name -> (stream, signed, nbits)           the model names the error kind and the failing run
  PANICS     name -> (stream, signed, nbits, what the oracle reports[, its values])   inputs on which the reference panics
Model and oracle must agree on every VALID and MALFORMED case; the model alone must pass the reference's own RLE v2 vectors
(tests/kat_vectors.py)."""
import random
import zlib

import numpy as np

import kat_vectors as K
import oracle_lib as O
import rle2_enc as E
from rle2_enc import I64_MAX, I64_MIN, WIDTHS

VALID, MALFORMED, PANICS = {}, {}, {}
NBITS = (64, 32, 16)
N_MALFORMED = 1200  # values asked of a malformed stream: more than any of them holds


def wrap(v, nbits):
    v &= (1 << nbits) - 1
    return v - (1 << nbits) if v >> (nbits - 1) else v


def rnd(name):
    return random.Random(zlib.crc32(name.encode()))


def valid(name, stream, values, signed, nbits):
    assert name not in VALID, name
    VALID[name] = (bytes(stream), [int(v) for v in values], signed, nbits)


def malformed(name, stream, signed, nbits):
    assert name not in MALFORMED, name
    MALFORMED[name] = (bytes(stream), signed, nbits)


def tag(nbits, signed):
    return "i%d%s" % (nbits, "s" if signed else "u")


# ---- DIRECT ---------------------------------------------------------------------------------------------------------------------
DIRECT_LENGTHS = (1, 2, 7, 8, 9, 63, 64, 65, 511, 512)
for nbits in NBITS:
    for signed in (True, False):
        for code, W in enumerate(WIDTHS):
            if W > nbits:
                # wider than N: OutOfSpec before the length byte is looked at
                malformed("direct/w%d too wide/%s" % (W, tag(nbits, signed)), E.direct([1, 2, 3], code, signed), signed, nbits)
                continue
            for L in DIRECT_LENGTHS:
                name = "direct/w%d/n%d/%s" % (W, L, tag(nbits, signed))
                r = rnd(name)
                vals = [r.randrange(-(1 << (W - 1)), 1 << (W - 1)) if signed else r.randrange(1 << W) for _ in range(L)]
                valid(name, E.direct(vals, code, signed), [wrap(v, nbits) for v in vals], signed, nbits)
            # all-ones and alternating payloads, given as the packed words themselves
            for what, words in (("ones", [(1 << W) - 1] * 9), ("alternating", [int("10" * W, 2) >> W if i & 1 else int("01" * W, 2) >> W for i in range(9)])):
                want = [wrap((u >> 1) ^ -(u & 1), nbits) if signed else wrap(u, nbits) for u in words]
                valid("direct/w%d/%s/%s" % (W, what, tag(nbits, signed)), E.direct(words, code, False), want, signed, nbits)
valid("direct/w64/i64 extremes/i64s", E.direct([I64_MIN, I64_MAX, -1, 0, I64_MAX, I64_MIN], 31, True), [I64_MIN, I64_MAX, -1, 0, I64_MAX, I64_MIN], True, 64)
valid("direct/w32/i32 extremes/i32s", E.direct([-(1 << 31), (1 << 31) - 1, -1], 27, True), [-(1 << 31), (1 << 31) - 1, -1], True, 32)
valid("direct/w16/i16 extremes/i16s", E.direct([-(1 << 15), (1 << 15) - 1, -1], 15, True), [-(1 << 15), (1 << 15) - 1, -1], True, 16)

# ---- SHORT_REPEAT ---------------------------------------------------------------------------------------------------------------
for nbits in NBITS:
    for signed in (True, False):
        for nb in range(1, 9):
            if nb * 8 > nbits:
                malformed("short_repeat/%d bytes too wide/%s" % (nb, tag(nbits, signed)), E.short_repeat(1, 5, nb, signed), signed, nbits)
                continue
            for count in range(3, 11):
                lo, hi = (-(1 << (8 * nb - 1)), (1 << (8 * nb - 1)) - 1) if signed else (0, (1 << 8 * nb) - 1)
                v = (lo, hi, rnd("sr%d%d" % (nb, count)).randrange(lo, 0) if signed else hi >> 1)[count % 3]
                valid("short_repeat/%d bytes/x%d/%s" % (nb, count, tag(nbits, signed)), E.short_repeat(v, count, nb, signed), [wrap(v, nbits)] * count, signed, nbits)

# ---- DELTA, fixed (width code 0) ------------------------------------------------------------------------------------------------
for nbits in NBITS:
    lo, hi = -(1 << (nbits - 1)), (1 << (nbits - 1)) - 1
    big = 1 << (nbits - 2)
    for L in (1, 2, 3, 512):
        for step in (0, 1, -1, big, -big):
            if abs(step) == big and L == 512:
                continue  # leaves N at the third step: among the malformed ones below
            base = lo if step > 0 else hi  # 2 * big steps from one end of N stay inside it
            name = "delta fixed/n%d/step %+d/%s" % (L, step, tag(nbits, True))
            valid(name, E.delta(base, step, 0, [], L, True), [base + i * step for i in range(L)], True, nbits)
    for step in (1, -1, big, -big):
        L = 512 if abs(step) == 1 else 4
        end = hi if step > 0 else lo
        # the last value is N's very end; one step further (the twin) leaves N at the last step only
        valid("delta fixed/ends at the limit/step %+d/%s" % (step, tag(nbits, True)), E.delta(end - (L - 1) * step, step, 0, [], L, True),
              [end - (L - 1 - i) * step for i in range(L)], True, nbits)
        malformed("delta fixed/overflow on the last step/step %+d/%s" % (step, tag(nbits, True)), E.delta(end - (L - 2) * step, step, 0, [], L, True), True, nbits)
        malformed("delta fixed/overflow on the first step/step %+d/%s" % (step, tag(nbits, True)), E.delta(end, step, 0, [], L, True), True, nbits)
    malformed("delta fixed/n512/step %+d leaves N/%s" % (big, tag(nbits, True)), E.delta(lo, big, 0, [], 512, True), True, nbits)
valid("delta fixed/unsigned near 2^63/i64u", E.delta((1 << 63) - 5, 1, 0, [], 5, False), [(1 << 63) - 5 + i for i in range(5)], False, 64)
malformed("delta fixed/unsigned past 2^63/i64u", E.delta((1 << 63) - 5, 1, 0, [], 7, False), False, 64)
# an unsigned base of 2^63 and more is a negative i64 (the varint's 64 bits as they are)
valid("delta fixed/unsigned base 2^63/i64u", E.delta(1 << 63, 1, 0, [], 3, False), [I64_MIN, I64_MIN + 1, I64_MIN + 2], False, 64)
malformed("delta/base varint too long/i64s", bytes([0xC0, 0x02]) + b"\x80" * 10 + b"\x00" + b"\x02", True, 64)
malformed("delta/base varint too long/i32s", bytes([0xC0, 0x02]) + b"\x80" * 5 + b"\x00" + b"\x02", True, 32)
malformed("delta/base varint too long/i16s", bytes([0xC0, 0x02]) + b"\x80" * 3 + b"\x00" + b"\x02", True, 16)
# the last varint byte that still fits: its bits above N fall off (0x7f at shift 14 of an i16: two bits stay)
valid("delta/base varint top bits fall off/i16u", bytes([0xC0, 0x00, 0x80, 0x80, 0x7F, 0x00]), [wrap(0x7F << 14, 16)], False, 16)

# ---- DELTA, packed --------------------------------------------------------------------------------------------------------------
for nbits in NBITS:
    lo, hi = -(1 << (nbits - 1)), (1 << (nbits - 1)) - 1
    for code in range(1, 32):
        W = WIDTHS[code]
        for L in (2, 3, 20):
            for first in (7, 0, -7):
                for signed in (True, False):
                    name = "delta packed/w%d/n%d/first %+d/%s" % (W, L, first, tag(nbits, signed))
                    r = rnd(name)
                    cap = min((1 << W) - 1, (1 << (nbits - 2)) // 32)
                    mags = [r.randrange(cap + 1) for _ in range(L - 2)]
                    if L == 20:
                        mags[3] = cap  # all of the width's bits, where N has room for them
                    sign = 1 if first > 0 else -1  # zero: subtract (delta.rs:77-82)
                    base = 0 if signed or sign > 0 else sum(mags) + 7
                    want, acc = [base, base + first], base + first
                    for m in mags:
                        acc += sign * m
                        want.append(acc)
                    valid(name, E.delta(base, first, code, mags, L, signed), want, signed, nbits)
    # one step that reaches N's end exactly; its twin goes one further, at the last value
    for first, end in ((5, hi), (-5, lo), (0, lo)):
        sign = 1 if first > 0 else -1
        base = end - sign * (abs(first) + 3 + 4)
        valid("delta packed/ends at the limit/first %+d/%s" % (first, tag(nbits, True)), E.delta(base, first, 3, [3, 4], 4, True),
              [base, base + first, base + first + sign * 3, end], True, nbits)
        malformed("delta packed/overflow at the last value/first %+d/%s" % (first, tag(nbits, True)), E.delta(base, first, 3, [3, 5], 4, True), True, nbits)
    malformed("delta packed/overflow at the second value/%s" % tag(nbits, True), E.delta(hi, 1, 3, [0, 0], 4, True), True, nbits)
# deltas are 64-bit whatever N is: a 64-bit magnitude with its top bit set is a NEGATIVE i64, and subtracting it adds
valid("delta packed/w64/magnitude with the top bit/i64s", E.delta(0, -1, 31, [(1 << 64) - 3], 3, True), [0, -1, 2], True, 64)
valid("delta packed/w64/magnitude with the top bit/i32s", E.delta(0, 1, 31, [(1 << 64) - 3], 3, True), [0, 1, -2], True, 32)
valid("delta packed/unsigned near 2^63/i64u", E.delta((1 << 63) - 20, 5, 7, [6, 8], 4, False), [(1 << 63) - 20, (1 << 63) - 15, (1 << 63) - 9, (1 << 63) - 1], False, 64)
malformed("delta packed/unsigned past 2^63/i64u", E.delta((1 << 63) - 20, 5, 7, [6, 9], 4, False), False, 64)
# a first delta wider than N is fine as long as the sum fits N
valid("delta packed/first delta wider than N/i16s", E.delta(-30000, 60000, 3, [1], 3, True), [-30000, 30000, 30001], True, 16)

# ---- PATCHED_BASE ---------------------------------------------------------------------------------------------------------------
def patched_values(reduced, W, base, entries, nbits, pw):
    """what the header fields mean: entry k patches the slot `gap` behind the slot entry k - 1 patched (fillers add 255)"""
    out = [wrap(v, nbits) for v in reduced]
    patched, at = {}, 0
    for gap, patch in entries:
        at += gap
        if not (gap == 255 and patch == 0):
            patched[at] = patch
    for i, v in enumerate(out):
        out[i] = wrap((v | wrap(patched[i] << W, nbits)) + base, nbits) if i in patched else v + base
    return out


for nbits in NBITS:
    hi = (1 << (nbits - 1)) - 1
    # every base width, positive and negative (sign bit set), zero and "minus zero"
    for bb in range(1, 9):
        mag = min((1 << (8 * bb - 1)) - 1, hi - 4000)
        for base in (mag, -mag, 0, "-0"):
            b = 0 if base == "-0" else base
            reduced = list(range(10))
            valid("patched/base of %d bytes/%s/%s" % (bb, base if isinstance(base, str) else "%+d" % base, tag(nbits, True)),
                  E.patched_base(reduced, 3, base, bb, 3, 3, [(4, 9)], True), patched_values(reduced, 4, b, [(4, 9)], nbits, 4), True, nbits)
    # a base written in more bytes than N has: what is above N falls off (N::from_i64), sign-magnitude undone first
    for bb in range(nbits // 8 + 1, 9):
        for sign in (1, -1):
            base = sign * ((1 << (8 * bb - 2)) + (1 << nbits) + 1234)
            reduced = list(range(10))
            valid("patched/base of %d bytes wider than N/%+d/%s" % (bb, sign, tag(nbits, True)), E.patched_base(reduced, 3, base, bb, 3, 3, [(4, 9)], True),
                  patched_values(reduced, 4, sign * 1234, [(4, 9)], nbits, 4), True, nbits)
    # every patch width x every gap width whose sum is at most 64: two entries, so that an entry of the wrong width moves the second
    for pcode, PW in enumerate(WIDTHS):
        for gw in range(1, 9):
            name = "patched/patch %d + gap %d = %d bits/%s" % (PW, gw, PW + gw, tag(nbits, True))
            reduced = [i % 16 for i in range(12)]
            if PW + gw > 64:
                malformed(name, E.patched_base(reduced, 3, 100, 2, pcode, gw, [(1, 1), (1, 1)], True), True, nbits)
                continue
            g = (1 << gw) - 1 if gw < 4 else 5
            entries = [(1, (1 << PW) - 1), (g, (1 << (PW - 1)) | 1)]
            valid(name, E.patched_base(reduced, 3, 100, 2, pcode, gw, entries, True), patched_values(reduced, 4, 100, entries, nbits, PW), True, nbits)
    # the entry's spare bits belong to the gap: 20 + 5 bits are written as 26, and the gap read is 6 bits wide
    entries = [(40, 3), (33, 1)]
    reduced = [i & 255 for i in range(100)]
    valid("patched/gap in the entry's spare bit/%s" % tag(nbits, True), E.patched_base(reduced, 7, 50, 1, 19, 5, entries, True),
          patched_values(reduced, 8, 50, entries, nbits, 20), True, nbits)
    # patch lists (512 values of 8 bits, patches of 4 bits, gaps of 8 bits)
    reduced = [(i * 7) & 255 for i in range(512)]
    lists = {
        "one entry": [(100, 5)],
        "31 entries": [(i + 1, 1 + i % 15) for i in range(31)],
        "first and last slot": [(0, 7), (255, 0), (255, 0), (1, 9)],
        "adjacent slots": [(17, 3), (1, 4), (1, 5)],
        "one filler": [(255, 0), (2, 6)],
        "two fillers": [(255, 0), (255, 0), (1, 6)],
        "three fillers, then behind the run": [(255, 0), (255, 0), (255, 0), (1, 6)],
        "filler between patches": [(3, 2), (255, 0), (200, 6)],
        "behind the run": [(5, 1), (254, 2), (254, 3)],
        "gap 255 with a patch is no filler": [(255, 1), (255, 2)],
    }
    for what, entries in lists.items():
        valid("patched/list: %s/%s" % (what, tag(nbits, True)), E.patched_base(reduced, 7, -100, 1, 3, 8, entries, True),
              patched_values(reduced, 8, -100, entries, nbits, 4), True, nbits)
    # a patched slot wraps (the patch sets N's top bits), its unpatched neighbours stay inside N ...
    W, wcode = (8, 7)
    top = nbits - 8 - 1  # patch bit that lands on N's sign bit
    pcode = WIDTHS.index(E.closest_fixed_bits(top + 1))
    reduced = [1, 2, 3, 4, 5, 6]
    entries = [(2, 1 << top)]
    valid("patched/patched slot wraps/%s" % tag(nbits, True), E.patched_base(reduced, wcode, -10, 1, pcode, 2, entries, True),
          patched_values(reduced, 8, -10, entries, nbits, WIDTHS[pcode]), True, nbits)
    # ... and beside an unpatched slot that overflows (base near N's end): the wrapping one passes, the run fails at the other
    base_bytes = nbits // 8
    malformed("patched/patched slot wraps beside an unpatched slot that overflows/%s" % tag(nbits, True),
              E.patched_base([0, 0, 200, 0, 0, 250], wcode, hi - 220, base_bytes, pcode, 2, [(2, 1 << top)], True), True, nbits)
    valid("patched/patched slot wraps where an unpatched one would overflow/%s" % tag(nbits, True),
          E.patched_base([0, 0, 250, 0, 0, 220], wcode, hi - 220, base_bytes, 0, 2, [(2, 0)], True),
          [hi - 220, hi - 220, wrap(hi + 30, nbits), hi - 220, hi - 220, hi], True, nbits)
# a patch for 64-bit values cannot be shifted: OutOfSpec when it is due, and not if it never is
malformed("patched/w64 patch due/i64s", E.patched_base([1, 2, 3, 4], 31, 0, 1, 0, 3, [(2, 1)], True), True, 64)
valid("patched/w64 patch behind the run/i64s", E.patched_base([1, 2, 3, 4], 31, 0, 1, 0, 3, [(4, 1)], True), [1, 2, 3, 4], True, 64)
malformed("patched/patch 64 + gap 1 = 65 bits, no entries/i64s", E.patched_base([1, 2, 3], 3, 0, 1, 31, 1, [], True), True, 64)
# unsigned streams take the base's bytes as they are
valid("patched/unsigned base with the top bit/i64u", E.patched_base([0, 1, 2, 3], 3, 0x90, 1, 3, 2, [(1, 1)], False), [0x90, 0x90 + (1 | 1 << 4), 0x92, 0x93], False, 64)
valid("patched/unsigned 8-byte base with the top bit/i64u", E.patched_base([0, 1, 2], 3, (1 << 63) + 5, 8, 3, 2, [(3, 1)], False),
      [I64_MIN + 5, I64_MIN + 6, I64_MIN + 7], False, 64)

# ---- mixed streams: every ordered pair of the sub-encodings, short and long ---------------------------------------------------------
def sample_runs(nbits, long):
    n = 512 if long else 1
    r = rnd("mixed%d%d" % (nbits, long))
    dv = [r.randrange(-100, 100) for _ in range(n)]
    pv = [r.randrange(16) for _ in range(n)]
    return {
        "SR": (E.short_repeat(-3, 10 if long else 3, 1, True), [-3] * (10 if long else 3)),
        "DIRECT": (E.direct(dv, 7, True), dv),
        "PATCHED": (E.patched_base(pv, 3, 1000, 2, 5, 1, [(0, 33)], True), patched_values(pv, 4, 1000, [(0, 33)], nbits, 6)),
        "DELTA": (E.delta(-50, 2, 0, [], n, True), [-50 + 2 * i for i in range(n)]),
    }


for nbits in NBITS:
    for long in (False, True):
        runs = sample_runs(nbits, long)
        for a in runs:
            for b in runs:
                valid("mixed/%s then %s/%s/%s" % (a, b, "long" if long else "short", tag(nbits, True)), runs[a][0] + runs[b][0], runs[a][1] + runs[b][1], True, nbits)

# ---- a stream that ends inside a run: every cut of one run of each kind (behind a whole run, so that the failing run is the second)
def truncated_runs(nbits):
    big = 1 << (nbits - 3)
    return {
        "SR": E.short_repeat(-70000 if nbits > 16 else -7000, 4, 3 if nbits > 16 else 2, True),
        "DIRECT": E.direct([5, -6, 7], 11, True),
        "PATCHED": E.patched_base([1, 2, 3, 4, 5], 4, -300, 2, 9, 3, [(1, 700), (2, 9)], True),
        "DELTA fixed": E.delta(big, -(big >> 4), 0, [], 5, True),   # (a base varint of N's full length: 2, 4 or 9 bytes)
        "DELTA packed": E.delta(big, big >> 4, 9, [1, 2, 3], 5, True),
    }


TRUNCATED = {nbits: truncated_runs(nbits) for nbits in NBITS}
for nbits in NBITS:
    for what, run in TRUNCATED[nbits].items():
        for cut in range(len(run)):
            malformed("cut/%s at byte %d of %d/%s" % (what, cut, len(run), tag(nbits, True)), E.short_repeat(1, 3, 1, True) + run[:cut], True, nbits)
    malformed("cut/empty stream/%s" % tag(nbits, True), b"", True, nbits)

# ---- where the reference panics (the model says so; the oracle's answer is recorded: DESIGN.md section 2) -------------------------
PANICS.update({
    "patched/empty patch list": (E.patched_base([1, 2, 3], 3, 0, 1, 3, 1, [], True), True, 64, O.OUT_OF_SPEC),
    "patched/list of fillers only": (E.patched_base([1, 2, 3], 3, 0, 1, 3, 8, [(255, 0), (255, 0)], True), True, 64, O.OUT_OF_SPEC),
    "patched/fillers run off the list behind a patch": (E.patched_base([1, 2, 3], 3, 0, 1, 3, 8, [(1, 1), (255, 0)], True), True, 64, O.OUT_OF_SPEC),
    "delta packed/length 1": (E.delta(5, 1, 3, [], 1, True), True, 64, O.OUT_OF_SPEC),
    # abs() of i64::MIN: the oracle and the HIP path go on with the wrapped magnitude, as a release build of the reference does: it
    # is i64::MIN again, the sign says subtract, and -5 - i64::MIN = i64::MAX - 4 (a fifth field: the values the oracle must give)
    "delta fixed/first delta i64::MIN, length 1": (E.delta(-5, I64_MIN, 0, [], 1, True), True, 64, O.OK, [-5]),
    "delta fixed/first delta i64::MIN, length 2": (E.delta(-5, I64_MIN, 0, [], 2, True), True, 64, O.OK, [-5, I64_MAX - 4]),
    "delta fixed/first delta i64::MIN from 0": (E.delta(0, I64_MIN, 0, [], 2, True), True, 64, O.OUT_OF_SPEC),
    "delta packed/first delta i64::MIN": (E.delta(-5, I64_MIN, 3, [1], 3, True), True, 64, O.OK, [-5, I64_MAX - 4, I64_MAX - 5]),
    "patched/24-bit values into i16": (E.patched_base([1, 2, 3], 23, 0, 1, 3, 1, [(1, 1)], True), True, 16, O.OUT_OF_SPEC),
    "patched/40-bit values into i32": (E.patched_base([1, 2, 3], 28, 0, 1, 3, 1, [(1, 1)], True), True, 32, O.OUT_OF_SPEC),
    # not byte aligned: the oracle and the HIP path keep the low N bits, as a release build of the reference does
    "patched/17-bit values into i16": (E.patched_base([1, 2, 0x10003], 16, 0, 1, 3, 1, [(1, 1)], True), True, 16, O.OK, [1, 2, 3]),
})


def oracle(stream, n, signed, nbits):
    st, vals = O.int_rle(np.frombuffer(stream, dtype=np.uint8), n, version=2, signed=signed, nbits=nbits)
    return st, vals.tolist()


def test_the_tables_have_the_cases():
    print("rle2 cases: %d valid, %d malformed, %d on which the reference panics" % (len(VALID), len(MALFORMED), len(PANICS)))
    assert len(VALID) > 3000 and len(MALFORMED) > 150 and len(PANICS) >= 8


def test_model_and_oracle_agree_on_every_valid_case():
    wrong = []
    for name, (stream, want, signed, nbits) in VALID.items():
        got = E.decode(stream, len(want), signed, nbits)
        st, ovals = oracle(stream, len(want), signed, nbits)
        if got != want or st != O.OK or ovals != want:
            wrong.append((name, "model", got if isinstance(got, tuple) else got == want, "oracle", st, ovals == want))
        # ... and neither has anything left: one value more is the end of the stream
        more = E.decode(stream, len(want) + 1, signed, nbits)
        if not (isinstance(more, tuple) and more[0] == E.OUT_OF_SPEC and more[2] == want) or oracle(stream, len(want) + 1, signed, nbits)[0] != O.OUT_OF_SPEC:
            wrong.append((name, "behind the last run", more[:2] if isinstance(more, tuple) else "values"))
    assert not wrong, (len(wrong), wrong[:10])


def test_model_and_oracle_agree_on_every_malformed_case():
    wrong = []
    for name, (stream, signed, nbits) in MALFORMED.items():
        got = E.decode(stream, N_MALFORMED, signed, nbits)
        st, _ = oracle(stream, N_MALFORMED, signed, nbits)
        if not isinstance(got, tuple) or got[0] == E.PANICS or got[0] != st:
            wrong.append((name, "model", got[:2] if isinstance(got, tuple) else "values", "oracle", st))
            continue
        # the runs in front of the failing one are delivered: the oracle has exactly the model's values, and not one more
        before = got[2]
        st, ovals = oracle(stream, len(before), signed, nbits)
        if st != O.OK or ovals != before or oracle(stream, len(before) + 1, signed, nbits)[0] != got[0]:
            wrong.append((name, "values in front of the failing run", len(before), st))
    assert not wrong, (len(wrong), wrong[:10])


def test_the_truncated_runs_fail_as_the_text_says():
    """the end of the stream where a run starts is OutOfSpec (rle_v2/mod.rs:115-123), anywhere inside a run an IoError"""
    for name, (stream, signed, nbits) in MALFORMED.items():
        if name.startswith("cut/"):
            kind, run, before = E.decode(stream, N_MALFORMED, signed, nbits)
            first_run = name.startswith("cut/empty stream")
            assert (run, before) == ((0, []) if first_run else (1, [1, 1, 1])), name
            assert kind == (E.OUT_OF_SPEC if first_run or " at byte 0 " in name else E.IO_ERROR), (name, kind)


def test_model_passes_the_references_vectors():
    n = 0
    for name, data, want, signed, version, nbits in K.INT_RLE:
        if version == 2:
            assert E.decode(bytes(data), len(want), signed, nbits) == list(want), name
            n += 1
    assert n >= 12


def test_where_the_reference_panics():
    for name, case in PANICS.items():
        stream, signed, nbits, recorded = case[:4]
        got = E.decode(stream, N_MALFORMED, signed, nbits)
        assert isinstance(got, tuple) and got[0] == E.PANICS and got[1] == 0, (name, got)
        if recorded == O.OK:
            assert oracle(stream, len(case[4]), signed, nbits) == (O.OK, case[4]), (name, oracle(stream, len(case[4]), signed, nbits))
            assert oracle(stream, len(case[4]) + 1, signed, nbits)[0] == O.OUT_OF_SPEC, name  # and the stream ends there
        else:
            assert oracle(stream, N_MALFORMED, signed, nbits)[0] == recorded, (name, oracle(stream, N_MALFORMED, signed, nbits)[0], recorded)


def test_the_writers_write_what_the_references_vectors_hold():
    """the writers against bytes nobody here made (kat_vectors: the reference's own unit tests)"""
    assert E.short_repeat(10000, 5, 2, False) == bytes([0x0A, 0x27, 0x10])
    assert E.direct([23713, 43806, 57005, 48879], 15, False) == bytes([0x5E, 0x03, 0x5C, 0xA1, 0xAB, 0x1E, 0xDE, 0xAD, 0xBE, 0xEF])
    assert E.delta(2, 1, 1, [2, 2, 4, 2, 4, 2, 4, 6], 10, False) == bytes([0xC6 & ~4, 0x09, 0x02, 0x02]) + E.pack([2, 2, 4, 2, 4, 2, 4, 6], 2)
    assert E.delta(2, 1, 3, [2, 2, 4, 2, 4, 2, 4, 6], 10, False) == bytes([0xC6, 0x09, 0x02, 0x02, 0x22, 0x42, 0x42, 0x46])
    reduced = [30, 0, 20, 998000 & 255, 40, 50, 60, 70, 80, 90]
    assert E.patched_base(reduced, 7, 2000, 2, 11, 2, [(3, 998000 >> 8)], False) == bytes([0x8E, 0x09, 0x2B, 0x21, 0x07, 0xD0, 0x1E, 0x00, 0x14, 0x70, 0x28, 0x32, 0x3C, 0x46, 0x50, 0x5A, 0xFC, 0xE8])
