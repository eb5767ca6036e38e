"""Hand-built integer RLE v1 runs, byte RLE runs and boolean streams (tests/rle1_enc.py), judged without a GPU by the plain model
and by the CPU oracle.

Four tables, built once at import and shared with tests/test_gpu_rle1_runs.py:
  VALID         name -> (codec, stream, values, signed, nbits)   the values follow from the fields the case was written from,
                                                                 worked out here next to the case, not by the model
  MALFORMED     name -> (codec, stream, signed, nbits, kind, values in front)   streams that must fail, with the error kind and what
                                                                 is delivered in front of the failing run, again from the fields
  PANICS        name -> (codec, stream, signed, nbits, what the oracle reports)   inputs on which the reference panics: there are none
                                                                 (rle1_enc's docstring says why), the table is kept for its users
  WALK_STREAMS  name -> a function that builds (codec, stream, values, signed, nbits) of a stream of 2048 blocks and more for the
                                                                 walk-path tests (built when asked for: a MiB each)
codec is rle1_enc.V1, BYTE or BOOL; nbits is 64, 32 or 16 for RLE v1 and 8 for bytes and booleans (whose values are the bits).

The RLE v1 runs are the cross product counts x deltas x bases for every N, signed and unsigned, with the base's minimal varint;
the base varint's other forms (every padded length, bits above N in the last group) are crossed with the bases at three counts
and deltas each, the counts' and the deltas' ends among them -- the forms bear on the header parse, which neither count nor delta
enters, and the full product would be 70 000 runs."""
import functools
import random
import zlib

import numpy as np

import kat_vectors as K
import oracle_lib as O
import rle1_enc as E
from rle1_enc import BOOL, BYTE, V1

VALID, MALFORMED, PANICS, WALK_STREAMS = {}, {}, {}, {}
NBITS = (64, 32, 16)
N_MALFORMED = 1200  # values asked of a malformed stream: more than any of them holds
RLE_BLK = 512


def wrap(v, nbits):
    v &= (1 << nbits) - 1
    return v - (1 << nbits) if v >> (nbits - 1) else v


def limits(nbits):
    return -(1 << (nbits - 1)), (1 << (nbits - 1)) - 1


def value_of(u, signed, nbits):
    """what the varint payload u means: zigzag undone in N bits, or the N bits as they are"""
    u &= (1 << nbits) - 1
    return wrap((u >> 1) ^ -(u & 1), nbits) if signed else wrap(u, nbits)


def rnd(name):
    return random.Random(zlib.crc32(name.encode()))


def valid(name, codec, stream, values, signed, nbits):
    assert name not in VALID, name
    VALID[name] = (codec, bytes(stream), [int(v) for v in values], signed, nbits)


# valid runs in front of a malformed case ("each of the above also with valid runs in front"): they are delivered
FRONT = {V1: (E.v1_run(7, 0, 3, True), [7, 7, 7]), BYTE: (E.byte_run(7, 3), [7, 7, 7]), BOOL: (E.byte_run(0xA5, 3), [1, 0, 1, 0, 0, 1, 0, 1] * 3)}
FRONT_UNSIGNED = (E.v1_run(7, 0, 3, False), [7, 7, 7])


def malformed(name, codec, stream, signed, nbits, kind, before=()):
    """the case as it is, and behind valid runs"""
    assert name not in MALFORMED, name
    MALFORMED[name] = (codec, bytes(stream), signed, nbits, kind, [int(v) for v in before])
    f, fv = FRONT_UNSIGNED if codec == V1 and not signed else FRONT[codec]
    MALFORMED[name + "/behind valid runs"] = (codec, f + bytes(stream), signed, nbits, kind, fv + [int(v) for v in before])


def tag(nbits, signed):
    return "i%d%s" % (nbits, "s" if signed else "u")


# ---- RLE v1 runs ----------------------------------------------------------------------------------------------------------------
COUNTS = (3, 4, 64, 127, 128, 129, 130)
DELTAS = (-128, -127, -1, 0, 1, 127)


def base_payloads(nbits, signed):
    """the varint payloads of the bases: 0, +-1, 63, 64, every 2^(7k) and 2^(7k) - 1 below 2^N (where a varint grows by a byte;
    for N = 64 unsigned the last of them, 2^63, is the first base that reads negative), N's minimum and maximum"""
    lo, hi = limits(nbits)
    us = {E.zigzag(v) if signed else v & ((1 << nbits) - 1) for v in (0, 1, -1, 63, 64, lo, hi)}
    for k in range(1, E.max_groups(nbits)):
        us |= {1 << 7 * k, (1 << 7 * k) - 1}
    return sorted(u & ((1 << nbits) - 1) for u in us)


def run_case(name, stream, base, delta, count, signed, nbits):
    """valid when the last value is inside N (the values are monotonic), else OutOfSpec with nothing delivered"""
    lo, hi = limits(nbits)
    if lo <= base + (count - 1) * delta <= hi:
        valid(name, V1, stream, [base + i * delta for i in range(count)], signed, nbits)
    else:
        malformed(name, V1, stream, signed, nbits, E.OUT_OF_SPEC)


for nbits in NBITS:
    for signed in (True, False):
        mg = E.max_groups(nbits)
        for u in base_payloads(nbits, signed):
            base = value_of(u, signed, nbits)
            for count in COUNTS:
                for delta in DELTAS:
                    run_case("v1 run/cross/base %d x%d step %+d/%s" % (base, count, delta, tag(nbits, signed)),
                             bytes([count - 3, delta & 0xFF]) + E.varint(u), base, delta, count, signed, nbits)
            # the base varint's other forms: padded with 0x80 .. 0x00 to every length up to max_groups; bits above N in the last group
            # (steps towards zero, so that most of these are valid; run_case files the others under the malformed ones)
            down = base > 0
            for length in range(len(E.varint(u)) + 1, mg + 1):
                for count, delta in ((4, -1 if down else 1), (130, -128 if down else 127), (64, 0)):
                    run_case("v1 run/base %d in %d bytes x%d step %+d/%s" % (base, length, count, delta, tag(nbits, signed)),
                             bytes([count - 3, delta & 0xFF]) + E.varint(u, length), base, delta, count, signed, nbits)
            groups = [(u >> 7 * i) & 0x7F for i in range(mg)]
            groups[-1] |= (0x7F << (nbits - 7 * (mg - 1))) & 0x7F  # (N = 64, 32, 16: the last group holds 1, 4, 2 bits of N)
            for count, delta in ((130, -1 if down else 1), (3, -127 if down else 127), (128, 0)):
                run_case("v1 run/base %d with bits above N x%d step %+d/%s" % (base, count, delta, tag(nbits, signed)),
                         bytes([count - 3, delta & 0xFF]) + E.raw_varint(groups), base, delta, count, signed, nbits)
        # landing: the last value is N's maximum or minimum exactly; its twin starts one further and leaves N at the last step
        lo, hi = limits(nbits)
        for delta in (127, 1, -1, -128):
            end = hi if delta > 0 else lo
            for count in (3, 64, 130):
                base = end - (count - 1) * delta
                name = "v1 run/x%d step %+d lands on the limit/%s" % (count, delta, tag(nbits, signed))
                valid(name, V1, E.v1_run(base, delta, count, signed, None, nbits), [base + i * delta for i in range(count)], signed, nbits)
                malformed("v1 run/x%d step %+d lands one past the limit/%s" % (count, delta, tag(nbits, signed)), V1,
                          E.v1_run(base + (1 if delta > 0 else -1), delta, count, signed, None, nbits), signed, nbits, E.OUT_OF_SPEC)
            # where the run leaves N: at step 1, in the middle, at the last step (k values are inside N, the k-th step is not)
            for k in (1, 65, 129):
                malformed("v1 run/x130 step %+d leaves N at step %d/%s" % (delta, k, tag(nbits, signed)), V1,
                          E.v1_run(end - (k - 1) * delta, delta, 130, signed, None, nbits), signed, nbits, E.OUT_OF_SPEC)
# unsigned bases at and above 2^63 are negative numbers of N: stepping down from 2^63 leaves N, stepping up from 2^64 - 1 reaches 0
valid("v1 run/unsigned 2^63 steps up/i64u", V1, E.v1_run(1 << 63, 1, 3, False), [-(1 << 63), -(1 << 63) + 1, -(1 << 63) + 2], False, 64)
malformed("v1 run/unsigned 2^63 steps down/i64u", V1, E.v1_run(1 << 63, -1, 3, False), False, 64, E.OUT_OF_SPEC)
valid("v1 run/unsigned 2^64 - 1 steps to 0/i64u", V1, E.v1_run((1 << 64) - 1, 1, 3, False), [-1, 0, 1], False, 64)
malformed("v1 run/unsigned 2^63 - 1 steps past it/i64u", V1, E.v1_run((1 << 63) - 1, 1, 3, False), False, 64, E.OUT_OF_SPEC)
# runs that fit 64 bits but not N
malformed("v1 run/fits i64, not i32/i32s", V1, E.v1_run((1 << 31) - 100, 127, 3, True), True, 32, E.OUT_OF_SPEC)
malformed("v1 run/fits i64, not i16/i16s", V1, E.v1_run(-(1 << 15) + 100, -128, 130, True), True, 16, E.OUT_OF_SPEC)
malformed("v1 run/fits i64, not i32/i32u", V1, E.v1_run((1 << 31) - 2, 1, 4, False), False, 32, E.OUT_OF_SPEC)
malformed("v1 run/fits i64, not i16/i16u", V1, E.v1_run((1 << 15) - 2, 1, 4, False), False, 16, E.OUT_OF_SPEC)

# ---- RLE v1 literals ------------------------------------------------------------------------------------------------------------
LIT_COUNTS = (1, 2, 63, 64, 65, 127, 128)
for nbits in NBITS:
    for signed in (True, False):
        mg = E.max_groups(nbits)
        edge = [value_of(u, signed, nbits) for u in base_payloads(nbits, signed)]  # every varint-length boundary, N's extremes
        for n in LIT_COUNTS:
            t = tag(nbits, signed)
            vals = [edge[i % len(edge)] for i in range(n)]
            valid("v1 literals/x%d at the length boundaries/%s" % (n, t), V1, E.v1_literals(vals, signed, None, nbits), vals, signed, nbits)
            small = [(i * 7) % 64 for i in range(n)]
            s = E.v1_literals(small, signed)
            assert len(s) == 1 + n
            valid("v1 literals/x%d of one byte/%s" % (n, t), V1, s, small, signed, nbits)
            s = E.v1_literals(vals, signed, [mg] * n, nbits)
            assert len(s) == 1 + n * mg  # (128 x 10: the group of 1281 bytes)
            valid("v1 literals/x%d of %d bytes/%s" % (n, mg, t), V1, s, vals, signed, nbits)
            valid("v1 literals/x%d short and long/%s" % (n, t), V1, E.v1_literals(small, signed, [mg if i & 1 else 1 for i in range(n)]), small, signed, nbits)
    # one long varint among one-byte ones, at every payload offset around the 64-byte steps of the expansion (RT_V1_LIT): its
    # terminator then lies in the next step, and at offsets 64 and 128 it is the first varint of its step
    lo, hi = limits(nbits)
    for signed in ((True, False) if nbits == 64 else (True,)):
        for at in list(range(54, 65)) + list(range(118, 129)):
            vals = [(i * 5) % 64 for i in range(128)]
            lens = [1] * 128
            k = at
            if at == 128:  # (the group's last literal, behind one of two bytes)
                k, lens[0] = 127, 2
            vals[k] = (lo if signed else hi) if at & 1 else 5  # (lo zigzags to all ones: max_groups bytes unpadded; 5 is padded)
            lens[k] = E.max_groups(nbits)
            s = E.v1_literals(vals, signed, lens, nbits)
            assert s[1 + at] & 0x80 and not s[at] & 0x80 and len(s) == 128 + E.max_groups(nbits) + (at == 128)
            valid("v1 literals/long varint at payload offset %d/%s" % (at, tag(nbits, signed)), V1, s, vals, signed, nbits)
    # mixed streams
    valid("v1 mixed/run, literals, run/%s" % tag(nbits, True), V1, E.v1_run(-5, 2, 10, True) + E.v1_literals([lo, hi, 0], True) + E.v1_run(hi, -128, 130, True),
          [-5 + 2 * i for i in range(10)] + [lo, hi, 0] + [hi - 128 * i for i in range(130)], True, nbits)
    s, v = b"", []
    for i in range(40):
        s += E.v1_run(i, 1, 3, True) + E.v1_literals([-i], True)
        v += [i, i + 1, i + 2, -i]
    valid("v1 mixed/literals of 1 between runs of 3/%s" % tag(nbits, True), V1, s, v, True, nbits)

# ---- byte RLE: every count, header-like values and payloads, as the stream's last run and with 130 bytes and more behind it -----
BYTE_TAIL = (E.byte_literals(list(range(128))) + E.byte_run(5, 3), [wrap(i, 8) for i in range(128)] + [5] * 3)
assert len(BYTE_TAIL[0]) >= 130
EDGE_BYTES = (0x00, 0x01, 0x7F, 0x80, 0xFF)
for count in range(3, 131):
    v = EDGE_BYTES[count % 5]
    valid("byte run/x%d of 0x%02x/last" % (count, v), BYTE, E.byte_run(v, count), [wrap(v, 8)] * count, True, 8)
    valid("byte run/x%d of 0x%02x/followed" % (count, v), BYTE, E.byte_run(v, count) + BYTE_TAIL[0], [wrap(v, 8)] * count + BYTE_TAIL[1], True, 8)
for count in range(1, 129):
    what = count % 5
    payload = [(0x80, 0x00, 0x7F, 0xFF)[what]] * count if what < 4 else [(0x80, 0x00, 0x7F, 0xFF)[i % 4] for i in range(count)]
    valid("byte literals/x%d of headers/last" % count, BYTE, E.byte_literals(payload), [wrap(b, 8) for b in payload], True, 8)
    valid("byte literals/x%d of headers/followed" % count, BYTE, E.byte_literals(payload) + BYTE_TAIL[0], [wrap(b, 8) for b in payload] + BYTE_TAIL[1], True, 8)


# ---- boolean --------------------------------------------------------------------------------------------------------------------
def byte_rle_of(data):
    """a plain byte RLE writer for the boolean cases: runs of 3 and more equal bytes as runs, the rest as literals"""
    out, lit, i = bytearray(), [], 0

    def flush():
        for k in range(0, len(lit), 128):
            out.extend(E.byte_literals(lit[k:k + 128]))
        del lit[:]

    while i < len(data):
        j = i
        while j < len(data) and data[j] == data[i] and j - i < 130:
            j += 1
        if j - i >= 3:
            flush()
            out.extend(E.byte_run(data[i], j - i))
        else:
            lit.extend(data[i:j])
        i = j
    flush()
    return bytes(out)


BOOL_COUNTS = sorted({n for c in (8, 64, 512, 1024, 4096) for n in range(c - 7, c + 9)} | set(range(1, 9)))
for n in BOOL_COUNTS:
    r = rnd("bool%d" % n)
    forms = {
        "runs of 0x00 and 0xff": [0] * (n // 2) + [1] * (n - n // 2) if n >= 16 else [1] * n,
        "literal bytes": [r.randrange(2) for _ in range(n)],
    }
    for what, bits in forms.items():
        data = bytearray(E.bool_bytes(bits))
        if n % 8:
            data[-1] |= 0xFF >> (n % 8)  # the unused bits of the last byte: set, and never looked at
        valid("bool/%d bits/%s" % (n, what), BOOL, byte_rle_of(data), bits, True, 8)
    bits = forms["literal bytes"]
    valid("bool/%d bits/more in the stream than asked" % n, BOOL, byte_rle_of(E.bool_bytes(bits) + b"\xff\x00\xa5" * 3), bits, True, 8)

# ---- malformed: streams that end too early ---------------------------------------------------------------------------------------
for nbits in NBITS:
    MALFORMED["cut/empty stream/%s" % tag(nbits, True)] = (V1, b"", True, nbits, E.OUT_OF_SPEC, [])
MALFORMED["cut/empty stream/byte"] = (BYTE, b"", True, 8, E.IO_ERROR, [])
MALFORMED["cut/empty stream/bool"] = (BOOL, b"", True, 8, E.IO_ERROR, [])


def truncated_runs(nbits):
    """sample runs: a run whose base has N's full length, literals of mixed lengths (cuts inside a varint and between two)"""
    lo, hi = limits(nbits)
    return {"run": E.v1_run(lo, 1, 5, True), "literals": E.v1_literals([1, lo, -2, hi, 300], True)}


TRUNCATED = {nbits: truncated_runs(nbits) for nbits in NBITS}
for nbits in NBITS:
    for what, run in TRUNCATED[nbits].items():
        for cut in range(1, len(run)):
            # (a cut at byte 0 is the stream's clean end: OutOfSpec for RLE v1 -- the empty stream above, and behind valid runs here)
            malformed("cut/v1 %s at byte %d of %d/%s" % (what, cut, len(run), tag(nbits, True)), V1, run[:cut], True, nbits, E.IO_ERROR)
    malformed("cut/v1 run without its delta byte/%s" % tag(nbits, False), V1, bytes([5]), False, nbits, E.IO_ERROR)
    malformed("cut/v1 run without its base/%s" % tag(nbits, False), V1, bytes([5, 1]), False, nbits, E.IO_ERROR)
    malformed("cut/v1 literals inside a varint/%s" % tag(nbits, False), V1, bytes([0xFE, 0x05, 0x85]), False, nbits, E.IO_ERROR)
    malformed("cut/v1 literals between varints/%s" % tag(nbits, False), V1, bytes([0xFD, 0x05, 0x85, 0x01]), False, nbits, E.IO_ERROR)
TRUNCATED_BYTES = {"run": E.byte_run(9, 20), "literals": E.byte_literals(list(range(0x7A, 0x86)))}
for codec in (BYTE, BOOL):
    malformed("cut/%s run without its value" % codec, codec, TRUNCATED_BYTES["run"][:1], True, 8, E.IO_ERROR)
    for cut in range(1, len(TRUNCATED_BYTES["literals"])):
        malformed("cut/%s literals at byte %d" % (codec, cut), codec, TRUNCATED_BYTES["literals"][:cut], True, 8, E.IO_ERROR)
for count in range(1, 129):  # literals cut at each length
    malformed("cut/byte literals x%d, the last byte missing" % count, BYTE, E.byte_literals([0x80] * count)[:-1], True, 8, E.IO_ERROR)

# ---- malformed: varints too large ------------------------------------------------------------------------------------------------
for nbits in NBITS:
    mg = E.max_groups(nbits)
    for signed in (True, False):
        t = tag(nbits, signed)
        too_long = E.raw_varint([1] * (mg + 1))
        malformed("varint/base of %d bytes/%s" % (mg + 1, t), V1, bytes([0, 1]) + too_long + b"\x00", signed, nbits, E.VARINT_TOO_LARGE)
        # max_groups continuation bytes and the end: the byte that would be one too many is never there
        malformed("varint/base of %d bytes that goes on, then the end/%s" % (mg, t), V1, bytes([0, 1]) + E.raw_varint([1] * mg, range(mg)), signed, nbits, E.IO_ERROR)
        malformed("varint/base of %d bytes that goes on, and one byte/%s" % (mg, t), V1, bytes([0, 1]) + E.raw_varint([1] * (mg + 1), range(mg + 1)), signed, nbits, E.VARINT_TOO_LARGE)
        for k in (0, 1, 63, 64, 127):
            parts = [E.varint(i % 100) for i in range(128)]
            parts[k] = too_long
            malformed("varint/literal %d of 128 has %d bytes/%s" % (k, mg + 1, t), V1, b"\x80" + b"".join(parts), signed, nbits, E.VARINT_TOO_LARGE)
        # as long as it may be, in every literal: valid (the twin of the above)
        vals = [value_of((1 << nbits) - 1 - i, signed, nbits) for i in range(128)]
        valid("varint/128 literals of %d bytes, every bit of N/%s" % (mg, t), V1, b"\x80" + b"".join(E.varint((1 << nbits) - 1 - i) for i in range(128)), vals, signed, nbits)


# ---- streams for the walk-path tests (device/rle_scan.hip): 2048 blocks and more, under 4 MiB -------------------------------------
WALK_SIZE = 2100 * RLE_BLK


def walk_stream(name):
    def register(f):
        WALK_STREAMS[name] = functools.lru_cache(maxsize=None)(f)
        return WALK_STREAMS[name]
    return register


def _lits(codec, payload):
    """a literal group of one payload byte a value (below 0x80: in RLE v1 a signed one-byte varint), and its values"""
    if codec == V1:
        return bytes([0x100 - len(payload)]) + bytes(payload), [(b >> 1) ^ -(b & 1) for b in payload]
    return E.byte_literals(payload), [wrap(b, 8) for b in payload]


for _codec in (V1, BYTE):
    @walk_stream("regular/%s" % _codec)
    def _regular(codec=_codec):
        """full groups of 128 one-byte literals, 129 bytes each: the stride guess from the first run makes every block strong"""
        run, vals = _lits(codec, [(i * 3) % 120 for i in range(128)])
        n = WALK_SIZE // len(run) + 1
        return codec, run * n, vals * n, codec == V1, 64 if codec == V1 else 8

    @walk_stream("short/%s" % _codec)
    def _short(codec=_codec):
        """runs of 3 .. 10 and literal groups of 1 .. 8 in turn"""
        out, vals, i = bytearray(), [], 0
        while len(out) < WALK_SIZE:
            if i & 1:
                g, v = _lits(codec, [(i + 7 * k) % 100 for k in range(1 + (i >> 1) % 8)])
            elif codec == V1:
                g, v = E.v1_run(i % 90, 1, 3 + (i >> 1) % 8, True), [i % 90 + k for k in range(3 + (i >> 1) % 8)]
            else:
                g, v = E.byte_run(i % 90, 3 + (i >> 1) % 8), [i % 90] * (3 + (i >> 1) % 8)
            out += g
            vals += v
            i += 1
        return codec, bytes(out), vals, codec == V1, 64 if codec == V1 else 8

    @walk_stream("changing/%s" % _codec)
    def _changing(codec=_codec):
        """Literal groups of 101 .. 125 one-byte values of ever-changing size (102 .. 126 bytes, all multiples of 3): no block holds
        a full-run header (no byte is 0x80), no stride, every block is weak -- and a chain started at a wrong byte never meets the
        true one: a span's warm-up cannot find it.
        RLE v1: a payload byte (below 0x80) read as a header is a run: header, delta byte, a one-byte base -- 3 bytes, or 4 when
        the base's first byte is a true header (continuation bit set).  True headers lie at multiples of 3.  A wrong chain at
        residue 1 (mod 3) steps by 3 until a true header is its third byte, then by 4: residue 2.  At residue 2 a true header can
        only be its second byte (the delta): it steps by 3 for ever.  (Residue 0 lands on the next true header: merged.)
        Byte RLE: every payload byte is 0x00 (read as a header: a run, 2 bytes) or, where that hop would land on a true header,
        0xfe (2 literals, 3 bytes; groups are longer than 3 bytes, so that does not land on one): no wrong chain ever lands on a
        true header."""
        sizes, i, total = [], 0, 0
        while total < WALK_SIZE:
            sizes.append(102 + 3 * ((i * i * 5 + i * 3) % 9))
            total += sizes[-1]
            i += 1
        headers, p = set(), 0
        for s in sizes:
            headers.add(p)
            p += s
        out, vals, p = bytearray(), [], 0
        for k, s in enumerate(sizes):
            if codec == V1:
                payload = [(k + 3 * q) % 128 for q in range(s - 1)]
            else:
                payload = [0xFE if p + 1 + q + 2 in headers else 0x00 for q in range(s - 1)]
            g, v = _lits(codec, payload)
            out += g
            vals += v
            p += s
        return codec, bytes(out), vals, codec == V1, 64 if codec == V1 else 8


def hop(stream, p, codec):
    """what the block walks do at byte p (device/rle_scan.hip walk_block): the size of the run that starts there, 1 where none parses"""
    h = stream[p]
    if codec != V1:
        size = 2 if h < 0x80 else 1 + 0x100 - h
        return size if p + size <= len(stream) else 1
    if h < 0x80:
        q = p + 2
        while q < len(stream) and stream[q] & 0x80:
            q += 1
        return q + 1 - p if q < len(stream) and q - p - 2 < 10 else 1
    q, left, cur = p + 1, 0x100 - h, 0
    while left and q < len(stream):
        cur += 1
        if cur > 10:
            return 1
        if not stream[q] & 0x80:
            cur, left = 0, left - 1
        q += 1
    return q - p if not left else 1


def walk_total(stream):
    """the values the block walks count in a byte RLE stream (device/rle_scan.hip walk_block, the job's `total`): every run of the
    chain from byte 0, a byte at which no run parses -- a group that is cut, a run without its value: run_parse's answer, which
    the stream's last 129 bytes must get from hop_parse too -- counting nothing and hopping one byte"""
    p, total = 0, 0
    while p < len(stream):
        h = stream[p]
        size, n = (2, h + 3) if h < 0x80 else (1 + 0x100 - h, 0x100 - h)
        fits = p + size <= len(stream)
        total, p = total + (n if fits else 0), p + (size if fits else 1)
    return total


@functools.lru_cache(maxsize=None)
def decoy_stream(codec, every=8):
    """A run of 3 (2 or 3 bytes: no stride to guess from, every block searches), then groups of 127 literals of 128 bytes each --
    no block has a full-run header (0x80) of its own, every block is weak, and the true chain enters every block at offset F = 2
    (byte RLE) or 3 (RLE v1).  In every `every`-th block the payloads spell 0x80 four times, at block offsets 10, 10 + D, 10 + 2 D
    and 10 + 3 D, D the size a group of 128 literals has THERE: 129 for byte RLE (a header and 128 bytes, whatever they are); 130
    for RLE v1, where the true chain's header (0x81, 0x82) inside every such group reads as a continuation byte and joins the byte
    behind it, so that 128 terminators take 129 bytes behind the header.  In RLE v1 a payload byte 0x80 must be the first of a
    two-byte varint (0x80 0x00: zero, padded); the group that holds one has 126 literals and is 128 bytes long like the others.
    Why every decoy bites: the 0x80 at offset 10 is its block's first candidate, three more groups of 128 follow it at its size,
    plausible_header() passes and the block is strong at entry 10.  The block in front is weak and its chain leaves it at F, not
    at 10 and in front of it: rle_walk_kernel mode 1 asks whether the chain from F arrives at 10 (chain_hits) -- it goes from F to
    F + 128 -- and lets the strong block keep its entry.  The verify round then finds entry 10 against exit F.
    Why a false chain rejoins: it leaves the decoy block at 10 + 4 D - 512 and hops through payload bytes read as headers -- byte
    RLE: 0x00, a run, 2 bytes a hop, it keeps its parity, which is the true headers'; RLE v1: runs of 3 or 4 bytes, a residue
    modulo 3 that changes at true headers -- until it lands on a true header.  test_the_decoys_bite_on_paper follows every one of
    them with hop(): each is back on the true chain in front of the next decoy block.
    Returns (stream, values, blocks with a decoy)."""
    D = 130 if codec == V1 else 129
    first = E.v1_run(1, 0, 3, True) if codec == V1 else E.byte_run(1, 3)
    F = len(first)
    n_blocks = WALK_SIZE // RLE_BLK
    data = bytearray(first) + bytearray(n_blocks * RLE_BLK)
    decoys = [b for b in range(2, n_blocks - 2, every)]
    spots = {b * RLE_BLK + 10 + k * D for b in decoys for k in range(4)}
    vals = [1, 1, 1]
    for g in range(n_blocks * 4):
        p = F + 128 * g
        mine = [s for s in spots if p < s < p + 128]
        assert len(mine) <= 1 and p not in spots and p + 127 not in spots
        data[p] = 0x81 + (len(mine) if codec == V1 else 0)
        q = p + 1
        while q < p + 128:
            if q in spots:
                data[q] = 0x80
                vals.append(0 if codec == V1 else -128)
                q += 2 if codec == V1 else 1  # (RLE v1: 0x80 0x00)
            else:
                data[q] = 0 if codec != V1 else (q * 7) % 128
                vals.append((data[q] >> 1) ^ -(data[q] & 1))
                q += 1
    return bytes(data), vals, decoys


for _codec in (V1, BYTE):
    WALK_STREAMS["decoys/%s" % _codec] = functools.partial(lambda c: (c,) + decoy_stream(c)[:2] + (c == V1, 64 if c == V1 else 8), _codec)
    WALK_STREAMS["dense decoys/%s" % _codec] = functools.partial(lambda c: (c,) + decoy_stream(c, 2)[:2] + (c == V1, 64 if c == V1 else 8), _codec)


# ---- the tests ------------------------------------------------------------------------------------------------------------------
def model(codec, stream, n, signed, nbits):
    return E.decode_v1(stream, n, signed, nbits) if codec == V1 else E.decode_bytes(stream, n) if codec == BYTE else E.decode_bools(stream, n)


def oracle(codec, stream, n, signed, nbits):
    data = np.frombuffer(stream, dtype=np.uint8)
    if codec == V1:
        st, vals = O.int_rle(data, n, version=1, signed=signed, nbits=nbits)
    else:
        st, vals = (O.byte_rle if codec == BYTE else O.boolean)(data, n)
    return st, vals.tolist()


def test_the_tables_have_the_cases():
    per = {c: (sum(1 for v in VALID.values() if v[0] == c), sum(1 for v in MALFORMED.values() if v[0] == c)) for c in (V1, BYTE, BOOL)}
    print("rle1 cases: %d valid, %d malformed, %d on which the reference panics, %d walk streams; (valid, malformed) per codec: %s"
          % (len(VALID), len(MALFORMED), len(PANICS), len(WALK_STREAMS), per))
    # counted once from the catalogue above
    assert len(VALID) >= 6215 and len(MALFORMED) >= 1291 and len(WALK_STREAMS) == 10
    assert per[V1][0] >= 5463 and per[BYTE][0] >= 512 and per[BOOL][0] >= 240
    assert per[V1][1] >= 981 and per[BYTE][1] >= 283 and per[BOOL][1] >= 27
    assert not PANICS  # (nothing in the three decoders panics on input: rle1_enc's docstring)


def test_model_and_oracle_agree_on_every_valid_case():
    wrong = []
    for name, (codec, stream, want, signed, nbits) in VALID.items():
        got = model(codec, stream, len(want), signed, nbits)
        st, ovals = oracle(codec, stream, len(want), signed, nbits)
        if got != want or st != O.OK or ovals != want:
            wrong.append((name, "model", got[:2] if isinstance(got, tuple) else got == want, "oracle", st, ovals == want))
        if name.endswith("more in the stream than asked"):
            continue
        # ... and neither has anything left: one value more (booleans: one byte more) is the end of the stream
        more = len(want) + 1 if codec != BOOL else (len(want) + 7) // 8 * 8 + 1
        end = E.OUT_OF_SPEC if codec == V1 else E.IO_ERROR
        m = model(codec, stream, more, signed, nbits)
        if not (isinstance(m, tuple) and m[0] == end and m[2][:len(want)] == want) or oracle(codec, stream, more, signed, nbits)[0] != end:
            wrong.append((name, "behind the last run", m[:2] if isinstance(m, tuple) else "values", oracle(codec, stream, more, signed, nbits)[0]))
    assert not wrong, (len(wrong), wrong[:10])


def test_model_and_oracle_agree_on_every_malformed_case():
    wrong = []
    for name, (codec, stream, signed, nbits, kind, before) in MALFORMED.items():
        got = model(codec, stream, N_MALFORMED, signed, nbits)
        st, _ = oracle(codec, stream, N_MALFORMED, signed, nbits)
        if not isinstance(got, tuple) or got[0] != kind or got[2] != before or st != kind:
            wrong.append((name, "model", (got[0], got[1], len(got[2])) if isinstance(got, tuple) else "values", "oracle", st, "want", kind, len(before)))
            continue
        # the runs in front of the failing one are delivered: the oracle has exactly these values, and not one more
        st, ovals = oracle(codec, stream, len(before), signed, nbits)
        if st != O.OK or ovals != before or oracle(codec, stream, len(before) + 1, signed, nbits)[0] != kind:
            wrong.append((name, "values in front of the failing run", len(before), st))
    assert not wrong, (len(wrong), wrong[:10])


def test_the_cut_cases_fail_as_the_text_says():
    """RLE v1: the end of the stream where a run starts is OutOfSpec (rle_v1.rs:154-157), anywhere inside a run an IoError; byte RLE
    and booleans: an IoError at either place (byte.rs:232)"""
    n = 0
    for name, (codec, stream, signed, nbits, kind, before) in MALFORMED.items():
        if name.startswith("cut/"):
            got = model(codec, stream, N_MALFORMED, signed, nbits)
            behind = name.endswith("/behind valid runs")
            assert isinstance(got, tuple) and got[1] == (1 if behind else 0) and got[2] == before, name
            assert got[0] == (E.OUT_OF_SPEC if codec == V1 and "empty stream" in name else E.IO_ERROR), (name, got[0])
            n += 1
    assert n > 200
    # a stream of whole runs, asked for one value more than it holds: the clean end, behind valid runs
    for nbits in NBITS:
        assert E.decode_v1(FRONT[V1][0], 4, True, nbits) == (E.OUT_OF_SPEC, 1, [7, 7, 7])
    assert E.decode_bytes(FRONT[BYTE][0], 4) == (E.IO_ERROR, 1, [7, 7, 7])
    assert E.decode_bools(FRONT[BOOL][0], 25) == (E.IO_ERROR, 1, FRONT[BOOL][1])


def test_model_passes_the_references_vectors():
    n = 0
    for name, data, want, signed, version, nbits in K.INT_RLE:
        if version == 1:
            assert E.decode_v1(bytes(data), len(want), signed, nbits) == list(want), name
            n += 1
    assert n >= 6
    for name, data, want in K.BYTE_RLE:
        assert E.decode_bytes(bytes(data), len(want)) == [wrap(v, 8) for v in want], name
    for name, data, want in K.BOOLEAN:
        assert E.decode_bools(bytes(data), len(want)) == list(want), name
    assert len(K.BYTE_RLE) >= 4 and len(K.BOOLEAN) >= 3


def test_the_writers_write_what_the_references_vectors_hold():
    """the writers against bytes nobody here made (kat_vectors: the reference's own unit tests)"""
    assert E.v1_run(7, 0, 100, False) == bytes([0x61, 0x00, 0x07])
    assert E.v1_run(100, -1, 100, False) == bytes([0x61, 0xFF, 0x64])
    assert E.v1_run(150, -1, 130, False) + E.v1_run(20, -1, 20, False) == bytes([0x7F, 0xFF, 0x96, 0x01, 0x11, 0xFF, 0x14])
    assert E.v1_literals([2, 3, 6, 7, 11], False) == bytes([0xFB, 0x02, 0x03, 0x06, 0x07, 0x0B])
    assert E.v1_run(1, 1, 3, False) + E.v1_literals([0, 256], False) == bytes([0x00, 0x01, 0x01, 0xFE, 0x00, 0x80, 0x02])
    assert E.v1_run(2, 2, 4, False) + E.v1_run(1, 2, 4, False) + E.v1_literals([255], False) == bytes([0x01, 0x02, 0x02, 0x01, 0x02, 0x01, 0xFF, 0xFF, 0x01])
    assert E.byte_run(0, 100) == bytes([0x61, 0x00]) and E.byte_run(1, 4) == bytes([0x01, 0x01])
    assert E.byte_literals([0x44, 0x45]) == bytes([0xFE, 0x44, 0x45])
    assert E.byte_run(0, 10) + E.byte_literals([11, 12, 13]) + E.byte_run(5, 20) == bytes([0x07, 0x00, 0xFD, 0x0B, 0x0C, 0x0D, 0x11, 0x05])
    assert E.byte_literals(E.bool_bytes([0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1])) == bytes([0xFE, 0x44, 0x45])
    assert E.byte_literals(E.bool_bytes([1])) == bytes([0xFF, 0x80])
    assert byte_rle_of(E.bool_bytes([0] * 800)) == bytes([0x61, 0x00])


def test_model_agrees_with_the_generators():
    """the model on what the project's own encoders emit (orc_rust_amd.gen), a few seeded arrays"""
    from orc_rust_amd import gen
    rng = np.random.default_rng(11)
    arrays = [rng.integers(-1 << 62, 1 << 62, 3000), np.repeat(rng.integers(-1000, 1000, 40), rng.integers(1, 200, 40)),
              np.cumsum(rng.integers(-128, 128, 2000)), np.arange(5000) * -3, rng.integers(0, 5, 3000)]
    for i, a in enumerate(arrays):
        for signed in (True, False):
            v = a if signed else np.abs(a)
            assert E.decode_v1(bytes(gen.rle1(v, signed=signed)), len(v), signed, 64) == v.tolist(), (i, signed)
    for i, a in enumerate(arrays):
        b = (a & 0xFF).astype(np.uint8)
        assert E.decode_bytes(bytes(gen.byte_rle(b)), len(b)) == b.view(np.int8).tolist(), i
        bits = (a & 1).astype(np.uint8)[:len(a) - 3]
        assert E.decode_bools(bytes(gen.boolean(bits)), len(bits)) == bits.tolist(), i
        sizes = E.run_sizes(bytes(gen.byte_rle(b)), BYTE)
        assert sum(s[2] for s in sizes) == len(b) and sizes[-1][0] + sizes[-1][1] == len(gen.byte_rle(b))
    s = bytes(gen.rle1(arrays[1], signed=True))
    sizes = E.run_sizes(s, V1)
    assert sum(x[2] for x in sizes) == len(arrays[1]) and sizes[-1][0] + sizes[-1][1] == len(s)


def test_the_walk_streams_are_what_the_model_reads():
    for name, build in WALK_STREAMS.items():
        codec, stream, vals, signed, nbits = build()
        assert 2048 * RLE_BLK < len(stream) < 4 << 20, (name, len(stream))
        assert model(codec, stream, len(vals), signed, nbits) == vals, name
        if name.startswith("changing"):
            assert 0x80 not in stream, name  # no full-run header anywhere: no candidate, every block is weak
    for codec in (V1, BYTE):
        sizes = {s[1] for s in E.run_sizes(WALK_STREAMS["regular/%s" % codec]()[1], codec)}
        assert sizes == {129}, sizes


def test_the_changing_streams_never_let_a_wrong_chain_in():
    """(_changing's docstring) from every block's first byte that is no true header -- where a span's warm-up starts -- the walk's
    chain is followed for 40 blocks: RLE v1 chains at residue 0 may merge, no other chain ever does"""
    for codec in (V1, BYTE):
        _c, stream, _v, _s, _n = WALK_STREAMS["changing/%s" % codec]()
        headers = {s[0] for s in E.run_sizes(stream, codec)}
        stuck = 0
        for b in range(1, 2000, 7):
            p = b * RLE_BLK
            if p in headers or (codec == V1 and p % 3 == 0):
                continue
            end = p + 40 * RLE_BLK
            while p < end and p not in headers:
                p += hop(stream, p, codec)
            assert p >= end, (codec, b, p)
            stuck += 1
        assert stuck > 100, (codec, stuck)


def test_the_decoys_bite_on_paper():
    """(decoy_stream's docstring) every decoy passes the search's test, the true chain passes it by, and the false chain it sends on
    is back on the true chain in front of the next decoy block"""
    for codec in (V1, BYTE):
        for every in (8, 2):
            stream, _vals, decoys = decoy_stream(codec, every)
            headers = {s[0] for s in E.run_sizes(stream, codec)}
            assert len(decoys) >= 64 and (every != 2 or len(decoys) * 8 >= len(stream) // RLE_BLK)
            for b in decoys:
                b0 = b * RLE_BLK
                block = stream[b0:b0 + RLE_BLK]
                assert block.index(0x80) == 10 and b0 + 10 not in headers
                p = b0 + 10
                for _ in range(4):  # the candidate and the three headers behind it: 128 literals each
                    assert stream[p] == 0x80 and hop(stream, p, codec) == (130 if codec == V1 else 129), (codec, b, p)
                    p += hop(stream, p, codec)
                assert p > b0 + RLE_BLK and p not in headers
                while p not in headers:
                    p += hop(stream, p, codec)
                assert p < b0 + 2 * RLE_BLK, (codec, every, b, p - b0)
