"""Hand-built String / Binary columns, direct and dictionary-encoded, judged without a GPU by the plain model
(tests/string_model.py) and by the CPU oracle.

The tables, built once at import and shared with tests/test_gpu_string_cases.py:
  VALID           name -> direct case       every batch decodes
  MALFORMED       name -> direct case       a batch fails
  DICT_VALID      name -> dictionary case   every batch decodes
  DICT_MALFORMED  name -> dictionary case   the dictionary cannot be built, or a batch holds a key that is none
A case is a dict: its streams as the decoders read them (`streams`, `column`), the decoded values the model works on (`lengths` /
`keys`, `present`, `data` / `entries`), its batch sizes (`batches`) and `want(batch)`: ([(offsets, value bytes)] of the Ok batches,
None or (error kind, failing batch)).  That expectation is worked out here, next to the case, from the rows the case was written
from -- a list of byte strings, None for a null row -- and from the row the case breaks at: never by the model.  Model and
oracle must give it for every case at every batch size.

Where the HIP finishers (device/string_kernels.hip) cut their work: UTF-8 validation takes 16 bytes a thread and 4096 a workgroup,
with a fast path for a 16-byte vector of ASCII; the text of all batches is checked as one, a second pass re-creates the
per-batch view (a character split by a batch boundary fails the EARLIER batch, a row offset inside a character its own).  The
dictionary gather has four paths -- entries padded to 8 bytes (all <= 8 bytes, <= 1024 of them), staged in LDS (<= 2048 entries,
<= 8192 bytes, longest <= 64), cached offsets with a row-by-row copy (an entry of 65 bytes or more), uncached (more entries or
bytes) -- and keys of 1, 2 or 4 bytes (up to 255, up to 65535 entries, more); it works in tiles of 2048 rows, 8 rows a thread, and
stages 16 KiB of value bytes a round.

The reference's order of a batch's checks: OffsetOverflow (the i64 sum of the lengths above i32::MAX), then a negative length,
then value bytes past the end of DATA, then UTF-8 (Arrow errors all three)."""
import random
import zlib

import numpy as np

import gpu_util as G
import kat_vectors as K
import oracle_lib as O
import rle2_enc as R
import string_model as M
from orc_rust_amd import gen

VALID, MALFORMED, DICT_VALID, DICT_MALFORMED = {}, {}, {}, {}
ARROW, OVERFLOW = O.ARROW, O.OFFSET_OVERFLOW
STRING, BINARY, VARCHAR, CHAR = 7, 8, 16, 17
PRESENT, DATA, LENGTH, DICT = 0, 1, 2, 3
VECTOR, WORKGROUP, TILE, STAGE = 16, 4096, 2048, 16384
DICT_ROWS = TILE + 3  # a last tile of 3 rows; in batches of 999 a last batch of 53 = 6 * 8 + 5: a last thread with 5 rows
CONSTRUCTION = M.CONSTRUCTION


def rnd(name):
    return random.Random(zlib.crc32(name.encode()))


def u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8)


def unsigned_rle(values):
    """an unsigned RLE v2 stream: the project's writer for what a writer writes, DIRECT runs of 64-bit values (tests/rle2_enc.py)
    from the first value of 2^31 or more on"""
    values = [v & R.M64 for v in values]
    big = next((i for i, v in enumerate(values) if v >= 1 << 31), len(values))
    out = bytes(gen.rle2(np.array(values[:big], dtype=np.int64), signed=False)) if big else b""
    for at in range(big, len(values), 512):
        out += R.direct(values[at:at + 512], 31, False)
    return out


def nulls(n):
    """20 % nulls: every fifth row, from row 3 on"""
    return [0 if i % 5 == 3 else 1 for i in range(n)]


def expect(rows, batch):
    """[(offsets, value bytes)] of the batches of `rows` (bytes, None for a null row): the offsets restart at 0 in every batch"""
    out = []
    for r0 in range(0, len(rows), batch):
        offsets, parts = [0], []
        for r in rows[r0:r0 + batch]:
            parts.append(r or b"")
            offsets.append(offsets[-1] + len(parts[-1]))
        out.append((offsets, b"".join(parts)))
    return out


def wanted(rows, fail):
    """fail: None, or batch size -> (kind, failing batch); the batches in front of the failing one are those of `rows`"""
    def want(batch):
        if fail is None:
            return expect(rows, batch), None
        kind, fb = fail(batch)
        if fb == CONSTRUCTION:
            return [], (kind, fb)
        assert fb * batch <= len(rows)
        return expect(rows[:fb * batch], batch), (kind, fb)
    return want


def direct_case(table, name, rows, batches, fail=None, utf8=True, tail=(), data=None):
    """rows: the rows the column is written from; tail: LENGTH values of further non-null rows behind them (those a byte string
    cannot stand for); data: the DATA stream where it is not just the rows' bytes"""
    assert name not in VALID and name not in MALFORMED, name
    present = None if all(r is not None for r in rows) else [int(r is not None) for r in rows] + [1] * len(tail)
    lengths = [len(r) for r in rows if r is not None] + [M.i64(v) for v in tail]
    data = b"".join(r for r in rows if r is not None) if data is None else bytes(data)
    streams = [(1, LENGTH, u8(unsigned_rle(lengths))), (1, DATA, u8(data))]
    if present is not None:
        streams.append((1, PRESENT, u8(gen.boolean(np.array(present, dtype=np.uint8)))))
    table[name] = {"name": name, "n_rows": len(rows) + len(tail), "lengths": lengths, "present": present, "data": data, "utf8": utf8,
                   "column": {"column_id": 1, "orc_type": STRING if utf8 else BINARY, "encoding": 2}, "streams": streams,
                   "batches": tuple(batches), "rows": rows, "want": wanted(rows, fail)}


def dict_case(table, name, entries, keys, batches, present=None, fail=None, dict_lengths=None, dict_data=None, dictionary_size=None):
    """entries: the dictionary's byte strings; keys: one DATA value per non-null row; present: one 0/1 per row"""
    assert name not in DICT_VALID and name not in DICT_MALFORMED, name
    dict_lengths = [len(e) for e in entries] if dict_lengths is None else [M.i64(v) for v in dict_lengths]
    dict_data = b"".join(entries) if dict_data is None else bytes(dict_data)
    dictionary_size = len(dict_lengths) if dictionary_size is None else dictionary_size
    keys = [M.i64(k) for k in keys]
    it = iter(keys)
    flags = [1] * len(keys) if present is None else present
    rows = []  # (a key that is none leaves the rows at and behind it to `fail`)
    for f in flags:
        k = next(it) if f else None
        if k is not None and not 0 <= k < len(entries):
            break
        rows.append(None if k is None else entries[k])
    streams = [(1, DATA, u8(unsigned_rle(keys))), (1, LENGTH, u8(unsigned_rle(dict_lengths))), (1, DICT, u8(dict_data))]
    if present is not None:
        streams.append((1, PRESENT, u8(gen.boolean(np.array(present, dtype=np.uint8)))))
    table[name] = {"name": name, "n_rows": len(flags), "keys": keys, "present": present, "entries": entries, "dict_lengths": dict_lengths,
                   "dict_data": dict_data, "dictionary_size": dictionary_size,
                   "column": {"column_id": 1, "orc_type": STRING, "encoding": 3, "dictionary_size": dictionary_size}, "streams": streams,
                   "batches": tuple(batches), "rows": rows, "want": wanted(rows, fail)}


def at_row(row, kind=ARROW):
    """the batch of `row` fails"""
    return lambda batch: (kind, row // batch)


# ---- UTF-8: every lead byte class at its edges -----------------------------------------------------------------------------------
# smallest and largest code point of every class of lead byte; the second-byte rules of E0, ED, F0 and F4 at their valid edge
GOOD = ["C2 80", "DF BF", "E0 A0 80", "E0 BF BF", "E1 80 80", "EC BF BF", "ED 80 80", "ED 9F BF", "EE 80 80", "EF BF BF", "F0 90 80 80",
        "F0 BF BF BF", "F1 80 80 80", "F3 BF BF BF", "F4 80 80 80", "F4 8F BF BF"]
# one outside: an overlong form, a surrogate, beyond U+10FFFF; bytes that lead nothing; broken sequences
BAD = ["C1 BF", "C0 80", "E0 9F BF", "E0 80 80", "ED A0 80", "ED BF BF", "F0 8F BF BF", "F0 80 80 80", "F4 90 80 80", "F4 BF BF BF"]
BAD += ["%02X 80 80 80" % c for c in range(0xF5, 0x100)] + ["%02X" % c for c in (0xF5, 0xF8, 0xFC, 0xFE, 0xFF)]
BAD += ["80", "BF",             # a lone continuation byte
        "C3 A9 80", "41 80", "E2 82 AC 80", "F0 9F 98 80 80",  # a continuation byte after a complete character
        "80 80 80 80",          # four continuation bytes in a row
        "C3 41", "E2 41 41", "E2 82 41", "F0 41 41 41", "F0 9F 41 41", "F0 9F 98 41",  # a lead followed by ASCII too early
        "C3 C3 A9", "E2 C3 A9", "E2 82 C3 A9", "F0 9F C3 A9", "F0 9F 98 C3 A9"]       # a lead followed by another lead
CUT = ["C3", "E2", "E2 82", "F0", "F0 9F", "F0 9F 98"]  # the 2-, 3- and 4-byte forms cut after 1, 2 or 3 bytes


def hexb(s):
    return bytes.fromhex(s.replace(" ", ""))


for form in GOOD:
    x = hexb(form)
    assert len(x.decode("utf-8")) == 1  # (one character, to Python's strict decoder)
    direct_case(VALID, "utf8/" + form, [b"abc", b"de", b"", x, b"q" + x, x + x + b"z", x], (8192, 2, 1))
for form in BAD:
    x = hexb(form)
    # row 3 is the first to hold the bytes: alone in its row (invalid whatever follows), then inside ASCII
    direct_case(MALFORMED, "utf8/" + form, [b"abc", b"de", b"", x, b"q" + x + b"rs", b"end"], (8192, 2, 1), at_row(3))
    # ... and in the middle of a row only, ASCII on both sides
    direct_case(MALFORMED, "utf8/" + form + " inside a row", [b"abc", b"de", b"", b"fg", b"q" + x + b"rs", b"end"], (8192, 2, 1), at_row(4))
for form in CUT:
    x = hexb(form)
    # at the end of the text: the last bytes of the last row of the last batch
    direct_case(MALFORMED, "utf8/cut at the end of the text/" + form, [b"abc", b"de", b"fgh", b"ij", b"klm" + x], (8192, 2, 1), at_row(4))
    direct_case(MALFORMED, "utf8/cut at the end of a full vector/" + form, [b"abcdefgh", b"ijklmnopqrstuvwx"[:8 - len(x)] + x], (8192, 1), at_row(1))

# ---- UTF-8: characters across a thread's 16 bytes and a workgroup's 4096 -----------------------------------------------------------
SPLIT_CHARS = {2: "é".encode(), 3: "€".encode(), 4: "\U0001f600".encode()}
SPLITS = [(L, s) for L in (2, 3, 4) for s in range(1, L)]


def ascii_fill(n, salt=0):
    return bytes(0x61 + (i + salt) % 26 for i in range(n))


def boundary_text(boundary, placed):
    """placed: [(bytes, s)] -- each with its first s bytes in front of a multiple of `boundary` (of 64 at least apart, so that
    the vectors beside it are ASCII), ASCII everywhere else; returns (text, [position of each])"""
    out, at = bytearray(), []
    step = max(boundary, 64)
    for k, (x, s) in enumerate(placed):
        out += ascii_fill((k + 1) * step - s - len(out), k)
        at.append(len(out))
        out += x
    return bytes(out + ascii_fill(40)), at


def rows_of(text, row_bytes):
    return [text[i:i + row_bytes] for i in range(0, len(text), row_bytes)]


for boundary, row_bytes, batches in ((VECTOR, 50, (8192, 3)), (WORKGROUP, 1000, (8192, 4))):
    text, at = boundary_text(boundary, [(SPLIT_CHARS[L], s) for L, s in SPLITS])
    assert all((p + s) % boundary == 0 for p, (_, s) in zip(at, SPLITS))
    rows = rows_of(text, row_bytes)
    assert all(M.utf8_ok(r) for r in rows)  # (no row ends inside a character)
    direct_case(VALID, "boundary/%d" % boundary, rows, batches)
    # an invalid form at the same splits, a case each: a surrogate, a code point beyond U+10FFFF, a lead in front of ASCII
    for form, splits in (("ED A0 80", (1, 2)), ("F4 90 80 80", (1, 2, 3)), ("C3", (1,))):
        for s in splits:
            text, at = boundary_text(boundary, [(SPLIT_CHARS[3], 1), (hexb(form), s)])
            assert (at[1] + s) % boundary == 0
            rows = rows_of(text, row_bytes)
            assert all(M.utf8_ok(r) == (i != at[1] // row_bytes) for i, r in enumerate(rows)), (form, s)
            direct_case(MALFORMED, "boundary/%d/%s, %d in front" % (boundary, form, s), rows, batches, at_row(at[1] // row_bytes))

# ---- UTF-8: batch boundaries and row boundaries ----------------------------------------------------------------------------------
for L, s in [(L, s) for L in (3, 4) for s in range(1, L)]:
    x = SPLIT_CHARS[L]
    front = [b"aa", b"b", b"", b"cc", b"dd", "é".encode(), b"e", b"ff" + x[:s]]  # rows 0 .. 7: the character begins in row 7
    behind = [b"gg", b"h", b"ii", b"j"]
    # the first s bytes are the last of the batch of row 7, the rest the first of the batch of row 8 (batches of 4, 2, 1): the
    # EARLIER batch fails -- its bytes end inside a character; batches of 3 and 8192 hold both rows: the offset of row 8 fails them
    for what, middle in (("", [x[s:] + b"g"]), (", the next batch begins with a null row", [None, x[s:] + b"g"]),
                         (", the next batch begins with an empty row", [b"", x[s:] + b"g"])):
        direct_case(MALFORMED, "batch boundary/%d of %d bytes in front%s" % (s, L, what), front + middle + behind, (4, 2, 1, 3, 8192), at_row(7))
    # in the middle of a batch: Arrow for a String column, and nothing at all for a Binary column
    rows = [b"aa", b"b", b"", b"cc", b"dd", b"e" + x[:s], x[s:] + b"g", b"hh"]
    direct_case(MALFORMED, "row boundary/%d of %d bytes in front" % (s, L), rows, (4, 8192, 3), at_row(5))
    direct_case(VALID, "row boundary/%d of %d bytes in front, Binary" % (s, L), rows, (4, 8192, 3), utf8=False)
# an empty row at the very end of a batch: its offset is the batch's byte total, behind a multi-byte character
direct_case(VALID, "row boundary/empty rows at the end of a batch", [b"x", "日本".encode(), b"", b"", b"y", "\U0001f600".encode(), b"", b""], (4, 8192, 2, 8))
# pure ASCII but for the last byte of the last batch (the nonascii flag is raised by the very last byte looked at)
rows = [ascii_fill(13, i) for i in range(40)]
direct_case(MALFORMED, "ascii/the last byte is C3", rows + [b"abc\xc3"], (8192, 10), at_row(40))
direct_case(MALFORMED, "ascii/the last byte is C3 and ends a vector", rows + [b"abcdefg\xc3"], (8192, 10), at_row(40))
assert (13 * 40 + 4) % VECTOR and (13 * 40 + 8) % VECTOR == 0
direct_case(VALID, "ascii/all of it", rows, (8192, 10))
# DATA holds more than the rows consume: what lies behind is not text
rows = [b"abc", "€".encode(), b"de"]
direct_case(VALID, "surplus/an invalid byte behind the rows' bytes", rows, (8192, 2), data=b"".join(rows) + b"\xff\xc3\x80")
direct_case(VALID, "surplus/the rest of a character behind the rows' bytes", [b"abc", b"de"], (8192, 1), data=b"abcde\x82\xac")
# DATA cut inside a character: the rows' bytes are not there -- that is the error (Arrow as well: offsets past the values), and
# it is the batch of the row whose bytes are missing that fails
rows = [b"ab", b"cd", b"ef", b"gh", "x€".encode(), b"ij"]
direct_case(MALFORMED, "short DATA/cut inside a character", rows, (8192, 2, 1), at_row(4), data=b"".join(rows)[:10])
direct_case(MALFORMED, "short DATA/cut inside the last character", rows[:5], (8192, 2, 1), at_row(4), data=b"".join(rows[:5])[:-1])
direct_case(MALFORMED, "short DATA/cut in front of the last row", rows, (8192, 2, 1), at_row(5), data=b"".join(rows)[:-2])
direct_case(MALFORMED, "short DATA/no DATA at all", rows, (8192, 2), at_row(0), data=b"")
direct_case(MALFORMED, "short DATA/Binary", rows, (8192, 2, 1), at_row(5), utf8=False, data=b"".join(rows)[:-1])
# two errors in one column: the earlier batch is the one reported
G4 = [b"aa", b"bb", b"cc", b"dd"]  # a good batch of 4
direct_case(MALFORMED, "two errors/UTF-8 in batch 1, OffsetOverflow in batch 2", G4 + [b"e", b"\xff", b"f", b"g"], (4,), at_row(5), tail=[1 << 31, 1, 1, 1])
direct_case(MALFORMED, "two errors/OffsetOverflow in batch 1, UTF-8 in batch 2", G4, (4,), at_row(4, OVERFLOW), tail=[1, 1 << 31, 1, 1, 1, 1, 1, 1],
            data=b"aabbccddx\xff\xff\xff")
direct_case(MALFORMED, "two errors/UTF-8 in batches 1 and 2", G4 + [b"e", b"\xff", b"f", b"g", b"\x80", b"h"], (4,), at_row(5))
# two errors in ONE batch: the reference's order -- OffsetOverflow, then a negative length, then bytes past DATA, then UTF-8
direct_case(MALFORMED, "one batch/OffsetOverflow and invalid UTF-8", G4, (4,), at_row(4, OVERFLOW), tail=[1, 1 << 31], data=b"aabbccdd\xff")
direct_case(MALFORMED, "one batch/a negative length and invalid UTF-8", G4, (4,), at_row(4), tail=[1, -1], data=b"aabbccdd\xff")
direct_case(MALFORMED, "one batch/bytes past DATA and invalid UTF-8", G4, (4,), at_row(4), tail=[1, 5], data=b"aabbccdd\xff")

# ---- lengths, String and Binary --------------------------------------------------------------------------------------------------
EDGE_LENGTHS = (0, 1, 15, 16, 17, 4095, 4096, 4097)


def text_of(n, salt):
    """n bytes of text: ASCII with a two-byte character now and then (never across the end)"""
    out = bytearray(ascii_fill(n, salt))
    for p in range(5 + salt, n - 1, 37):
        out[p:p + 2] = "é".encode()
    return bytes(out)


rows = [text_of(n, i) for i, n in enumerate(EDGE_LENGTHS)]
assert [len(r) for r in rows] == list(EDGE_LENGTHS) and all(M.utf8_ok(r) for r in rows)
direct_case(VALID, "lengths/0 to 4097", rows, (8192, 3, 1))
direct_case(VALID, "lengths/0 to 4097, with nulls", [None, rows[7], rows[0], None] + rows + [None], (8192, 3, 1))
raw = [bytes(rnd("binary %d" % n).getrandbits(8) for _ in range(n)) for n in EDGE_LENGTHS]
direct_case(VALID, "lengths/0 to 4097, Binary", raw, (8192, 3, 1), utf8=False)
direct_case(VALID, "lengths/0 to 4097, Binary with nulls", raw[:3] + [None, None] + raw[3:], (8192, 3, 1), utf8=False)
for utf8, what in ((True, ""), (False, ", Binary")):
    direct_case(VALID, "lengths/all rows empty" + what, [b""] * 10, (8192, 4, 1), utf8=utf8)
    direct_case(VALID, "lengths/all rows null" + what, [None] * 10, (8192, 4, 1), utf8=utf8)
    direct_case(VALID, "lengths/a single row" + what, ["été".encode()], (8192, 1), utf8=utf8)
    direct_case(VALID, "lengths/a single empty row" + what, [b""], (8192, 1), utf8=utf8)
    direct_case(VALID, "lengths/a single null row" + what, [None], (8192, 1), utf8=utf8)
# the sum of a batch's lengths, over a DATA stream of a few bytes
SUMS = [("the sum is i32::MAX", [(1 << 31) - 2, 1], ARROW),            # not OffsetOverflow: DATA runs dry
        ("the sum is 2^31", [(1 << 31) - 1, 1], OVERFLOW),
        ("one length of 2^31", [1, 1 << 31], OVERFLOW),
        ("one length of 2^32", [1 << 32, 1], OVERFLOW),
        ("one length of 2^63 - 1", [(1 << 63) - 1], OVERFLOW),
        ("a length of -1", [1, (1 << 64) - 1, 1], ARROW),                 # the sum is 1
        ("-1 next to 2^31", [(1 << 64) - 1, 1 << 31], ARROW),             # the sum is i32::MAX: the negative length is what fails
        ("-1 next to 2^31 + 1", [(1 << 31) + 1, (1 << 64) - 1], OVERFLOW),  # the sum is 2^31
        ("2^63 - 1 twice: the sum wraps to -2", [(1 << 63) - 1, (1 << 63) - 1], ARROW),  # no length is negative: DATA runs dry
        ("-2^63 next to 2^63 - 1", [1 << 63, (1 << 63) - 1], ARROW)]      # the sum is -1
FRONT8 = [b"aa", "é".encode(), b"", b"cc", b"dd", b"e", "€".encode(), b"ff"]
for what, tail, kind in SUMS:
    for utf8, t in ((True, ""), (False, ", Binary")):
        direct_case(MALFORMED, "sums/%s, batch 0%s" % (what, t), [], (8192, 4), at_row(0, kind), utf8=utf8, tail=tail, data=b"abcdefg")
        # behind two good batches, which come out bit for bit
        direct_case(MALFORMED, "sums/%s, batch 2%s" % (what, t), FRONT8, (4,), at_row(8, kind), utf8=utf8, tail=tail, data=b"".join(FRONT8) + b"xyz")

# ---- dictionaries: a shape for every gather path and each side of every switch -----------------------------------------------------
WORDS = [b"", b"AIR", b"FOB", b"MAIL", b"REG AIR!", "héllo".encode(), "日本".encode(), b"RAIL", b"x", "\U0001f600".encode(), b""]
assert max(len(w) for w in WORDS) == 8 and WORDS[0] == WORDS[-1] == b""  # (one of exactly 8 bytes; the first and the last entry empty)


def short_entries(n, longest=8):
    """n entries of 0 .. `longest` bytes, ASCII"""
    return [ascii_fill((7 * i + 3) % (longest + 1), i) for i in range(n)]


SHAPES = {  # name -> (entries, gather path, key bytes)
    "11 entries of up to 8 bytes": (WORDS, "padded", 1),
    "an entry of 9 bytes": (WORDS + [b"123456789"], "staged", 1),
    "an entry of 64 bytes": (WORDS + [text_of(64, 3), b"z"], "staged", 1),
    "an entry of 65 bytes": (WORDS + [text_of(65, 4), b"z"], "cached offsets", 1),
    "100 entries of 33 bytes": ([text_of(33, i) for i in range(100)], "staged", 1),  # 2048 rows are 4 rounds of the stage and more
    "254 entries": (short_entries(254), "padded", 1),
    "255 entries": (short_entries(255), "padded", 1),
    "256 entries": (short_entries(256), "padded", 2),
    "1024 entries of up to 8 bytes": (short_entries(1024), "padded", 2),
    "1025 entries of up to 8 bytes": (short_entries(1025, 7), "staged", 2),
    "2048 entries": (short_entries(2048, 6), "staged", 2),
    "2049 entries": (short_entries(2049, 6), "uncached", 2),
    "65535 entries of 1 byte": ([bytes([0x41 + i % 26]) for i in range(65535)], "uncached", 2),
    "65536 entries of 1 byte": ([bytes([0x41 + i % 26]) for i in range(65536)], "uncached", 4),
    "8192 dictionary bytes": ([text_of(64, i) for i in range(128)], "staged", 1),
    "8193 dictionary bytes": ([text_of(64, i) for i in range(128)] + [b"!"], "uncached", 1),
    "all entries empty": ([b""] * 5, "padded", 1),
}
assert sum(len(e) for e in SHAPES["8192 dictionary bytes"][0]) == 8192 and sum(len(e) for e in SHAPES["8193 dictionary bytes"][0]) == 8193
assert sum(len(e) for e in SHAPES["1024 entries of up to 8 bytes"][0]) <= 8192 and max(len(e) for e in SHAPES["1024 entries of up to 8 bytes"][0]) == 8
assert sum(len(e) for e in SHAPES["2048 entries"][0]) <= 8192 < 2048 * 33


def shape_keys(name, n_entries, n):
    """n keys: the first and the last entry among them (at both ends, too), the rest drawn"""
    r = rnd("keys " + name)
    keys = [r.randrange(n_entries) for _ in range(n)]
    keys[0], keys[1], keys[n // 2], keys[-2], keys[-1] = n_entries - 1, 0, n_entries - 1, 0, n_entries - 1
    return keys


DICT_BATCHES = (8192, 999, 1)
for shape, (entries, _path, _kb) in SHAPES.items():
    dict_case(DICT_VALID, shape, entries, shape_keys(shape, len(entries), DICT_ROWS), DICT_BATCHES)
    flags = nulls(DICT_ROWS)
    dict_case(DICT_VALID, shape + ", with nulls", entries, shape_keys(shape + " nulls", len(entries), sum(flags)), DICT_BATCHES, present=flags)
dict_case(DICT_VALID, "no entries, only null rows", [], [], DICT_BATCHES, present=[0] * DICT_ROWS)
# text in a dictionary: every valid edge of the lead byte classes; characters across the 16-byte and 4096-byte cuts of its bytes
dict_case(DICT_VALID, "utf8/every valid edge", [hexb(form) for form in GOOD], shape_keys("edges", len(GOOD), 100), (8192, 7))
for boundary, row_bytes in ((VECTOR, 50), (WORKGROUP, 1000)):
    entries = VALID["boundary/%d" % boundary]["rows"]
    dict_case(DICT_VALID, "utf8/boundary/%d" % boundary, entries, shape_keys("boundary %d" % boundary, len(entries), 60), (8192, 7))

# keys that are none: an Arrow error in the batch of that row, the batches in front intact
BAD_ROW = 1500
for what, n_entries, key in (("a key equal to the dictionary size", 11, 11), ("key 255 with 255 entries", 255, 255),
                             ("key 65535 with 65535 entries", 65535, 65535), ("key 2048 with 2048 entries", 2048, 2048),
                             ("key 2049 with 2049 entries", 2049, 2049), ("key 65536 with 65536 entries", 65536, 65536),
                             ("a key of 2^31", 11, 1 << 31), ("a key of 2^32", 11, 1 << 32), ("a key of 2^32 with 65536 entries", 65536, 1 << 32),
                             ("a key of 2^63", 11, 1 << 63), ("a key of -1", 300, (1 << 64) - 1)):
    entries = WORDS if n_entries == 11 else [bytes([0x41 + i % 26]) * (1 + i % 3) for i in range(n_entries)]
    keys = shape_keys(what, n_entries, DICT_ROWS)
    keys[BAD_ROW] = key
    dict_case(DICT_MALFORMED, "keys/" + what, entries, keys, (8192, 999), fail=at_row(BAD_ROW))
flags = nulls(DICT_ROWS)
keys = shape_keys("bad key under nulls", 11, sum(flags))
keys[sum(flags[:BAD_ROW])] = 11  # the key of row 1500 (not a null row)
assert flags[BAD_ROW]
dict_case(DICT_MALFORMED, "keys/a key equal to the dictionary size, with nulls", WORDS, keys, (8192, 999, 100), present=flags, fail=at_row(BAD_ROW))
dict_case(DICT_MALFORMED, "keys/key 0 of no entries", [], [0] * 20, (8192, 8), fail=at_row(0))
dict_case(DICT_MALFORMED, "keys/key 0 of no entries, behind null rows", [], [0], (8192, 8), present=[0] * 19 + [1], fail=at_row(19))


# dictionaries that cannot be built: the column fails before batch 0, whatever the keys
def broken(name, kind, entries=(), **kw):
    dict_case(DICT_MALFORMED, "dictionary/" + name, list(entries), [0] * 30, (8192, 8), fail=lambda batch: (kind, CONSTRUCTION), **kw)


# (the lengths are summed as they are, 2^31 + -5 is below i32::MAX: the negative length is what fails, string.rs:125-151)
broken("lengths 2^31 and -5", ARROW, dict_lengths=[1 << 31, (1 << 64) - 5], dict_data=b"abcdefg")
broken("lengths that sum to 2^31", OVERFLOW, dict_lengths=[(1 << 31) - 1, 1], dict_data=b"abcdefg")
broken("lengths that sum to i32::MAX", ARROW, dict_lengths=[(1 << 31) - 2, 1], dict_data=b"abcdefg")
broken("one length of 2^32", OVERFLOW, dict_lengths=[1, 1 << 32], dict_data=b"abcdefg")
broken("a single negative length", ARROW, dict_lengths=[3, (1 << 64) - 1, 2], dict_data=b"abcdefg")
broken("-1 next to 2^31 + 1", OVERFLOW, dict_lengths=[(1 << 31) + 1, (1 << 64) - 1], dict_data=b"abcdefg")
broken("2^63 - 1 twice: the sum wraps to -2", ARROW, dict_lengths=[(1 << 63) - 1, (1 << 63) - 1], dict_data=b"abcdefg")
broken("bytes one short of the sum", ARROW, WORDS, dict_data=b"".join(WORDS)[:-1])
broken("no bytes at all", ARROW, WORDS, dict_data=b"")
for form in BAD + CUT:
    broken("utf8/" + form, ARROW, [b"ab", hexb(form), b"cd"] if form not in CUT else [b"ab", b"cd" + hexb(form)])
broken("utf8/an entry boundary inside a character", ARROW, [b"a\xe2", b"\x82\xac", b"b"])
broken("utf8/an entry boundary inside a character, the last entry", ARROW, [b"a", b"b\xf0\x9f\x98", b"\x80"])
for boundary, row_bytes in ((VECTOR, 50), (WORKGROUP, 1000)):
    for form, s in (("ED A0 80", 1), ("F4 90 80 80", 3), ("C3", 1)):
        broken("utf8/boundary/%d/%s" % (boundary, form), ARROW, MALFORMED["boundary/%d/%s, %d in front" % (boundary, form, s)]["rows"])


# ---- the tests ------------------------------------------------------------------------------------------------------------------
def model_run(case, batch):
    if "keys" in case:
        return M.dictionary(case["dict_lengths"], case["dict_data"], case["dictionary_size"], case["keys"], case["present"], batch)
    return M.direct(case["lengths"], case["present"], case["data"], batch, case["utf8"])


def bits_of(bitmap, n):
    return None if bitmap is None else [bool(bitmap[i >> 3] >> (i & 7) & 1) for i in range(n)]


def oracle_run(case, batch, column=None):
    """the CPU oracle over the case's streams: ([(offsets, values, validity)], None or (kind, failing batch))"""
    oc = G.oracle_column(column or case["column"], case["streams"])
    if oc.status != O.OK:
        return [], (oc.status, CONSTRUCTION)
    out, left, b = [], case["n_rows"], 0
    while left > 0:
        n = min(batch, left)
        ob = oc.next_batch(n)
        if ob["status"] != O.OK:
            oc.close()
            return out, (ob["status"], b)
        assert ob["length"] == n
        out.append((ob["offsets"].tolist(), ob["values"], bits_of(ob["validity"], n)))
        left -= n
        b += 1
    oc.close()
    return out, None


def validity_want(case, batch):
    if case["present"] is None:
        return lambda b: None
    flags = case["present"]  # (a batch without a null row has no validity bitmap, string.rs:145-149)
    return lambda b: None if all(flags[b * batch:(b + 1) * batch]) else [bool(f) for f in flags[b * batch:(b + 1) * batch]]


def judge(table):
    wrong = []
    for name, case in table.items():
        for batch in case["batches"]:
            front, failure = case["want"](batch)
            valid = validity_want(case, batch)
            want = ([(o, v, valid(b)) for b, (o, v) in enumerate(front)], failure)
            for who, got in (("model", model_run(case, batch)), ("oracle", oracle_run(case, batch))):
                if got != want:
                    first = next((b for b, (x, y) in enumerate(zip(got[0], want[0])) if x != y), None)
                    wrong.append((name, batch, who, "failure", got[1], "want", failure, "batches", len(got[0]), len(front), "first wrong batch", first))
    assert not wrong, (len(wrong), wrong[:8])


def test_the_tables_have_the_cases():
    print("string cases: %d valid, %d malformed, %d valid dictionary, %d malformed dictionary"
          % (len(VALID), len(MALFORMED), len(DICT_VALID), len(DICT_MALFORMED)))
    assert len(VALID) >= 35 and len(MALFORMED) >= 150 and len(DICT_VALID) >= 2 * len(SHAPES) + 1 and len(DICT_MALFORMED) >= 60
    for form in BAD:
        assert not M.utf8_ok(hexb(form)), form
    for form in CUT:
        assert not M.utf8_ok(hexb(form)), form
    assert {"C1 BF", "C0 80", "E0 9F BF", "ED A0 80", "F0 8F BF BF", "F4 90 80 80"} <= set(BAD) and all("%02X 80 80 80" % c in BAD for c in range(0xF5, 0x100))
    assert {"C2 80", "E0 A0 80", "ED 9F BF", "EF BF BF", "F0 90 80 80", "F4 8F BF BF"} <= set(GOOD)
    for table in (VALID, MALFORMED, DICT_VALID, DICT_MALFORMED):
        for name, case in table.items():
            assert case["n_rows"] <= 20000 and sum(len(s[2]) for s in case["streams"]) < 300_000, name
            failing = [case["want"](b)[1] for b in case["batches"]]
            assert all((f is None) == (table in (VALID, DICT_VALID)) for f in failing), name
    # every sum edge in batch 0 and in batch 2, as String and as Binary
    assert sum(n.startswith("sums/") for n in MALFORMED) == 4 * len(SUMS) and len(SUMS) >= 9
    assert all(MALFORMED["sums/%s, batch 2" % w]["want"](4)[1] == (k, 2) and len(MALFORMED["sums/%s, batch 2" % w]["want"](4)[0]) == 2 for w, _, k in SUMS)


def test_the_dictionary_shapes_are_on_both_sides_of_every_switch():
    """the gather path and the key width each shape was written for, worked out again from the entries"""
    seen = set()
    for shape, (entries, path, key_bytes) in SHAPES.items():
        n, total, longest = len(entries), sum(len(e) for e in entries), max(len(e) for e in entries)
        if n > 2048 or total > 8192:
            got = "uncached"
        elif longest <= 8 and n <= 1024:
            got = "padded"
        else:
            got = "staged" if longest <= 64 else "cached offsets"
        assert got == path, (shape, got, path)
        assert key_bytes == (1 if n <= 255 else 2 if n <= 65535 else 4), shape
        seen.add((path, key_bytes))
        for name in (shape, shape + ", with nulls"):
            case = DICT_VALID[name]
            assert case["n_rows"] == DICT_ROWS and {0, n - 1} <= set(case["keys"]), name
    assert seen >= {("padded", 1), ("padded", 2), ("staged", 1), ("staged", 2), ("cached offsets", 1), ("uncached", 1), ("uncached", 2), ("uncached", 4)}
    # one staged shape's first tile holds more than a round of the stage, at a row size that does not divide it
    case = DICT_VALID["100 entries of 33 bytes"]
    assert sum(len(r) for r in case["rows"][:TILE]) > 4 * STAGE and STAGE % 33


def test_the_boundary_texts_place_what_they_say():
    for boundary in (VECTOR, WORKGROUP):
        text = b"".join(VALID["boundary/%d" % boundary]["rows"])
        seen = set()
        for L, s in SPLITS:
            for p in range(boundary - s, len(text), boundary):
                if text[p:p + L] == SPLIT_CHARS[L]:
                    seen.add((L, s))
                    # the vectors on both sides are ASCII apart from the character itself
                    lo, hi = p // 16 * 16 - 16, (p + L - 1) // 16 * 16 + 32
                    assert all(c < 0x80 for c in text[lo:p] + text[p + L:hi]), (boundary, L, s)
        assert seen == set(SPLITS), (boundary, sorted(set(SPLITS) - seen))


def test_the_streams_decode_to_the_values_the_model_is_given():
    """the LENGTH and DATA streams against the plain RLE v2 model (tests/rle2_enc.py), values of 2^63 and more read as negative"""
    for table in (VALID, MALFORMED, DICT_VALID, DICT_MALFORMED):
        for name, case in table.items():
            by_kind = {k: bytes(b) for _, k, b in case["streams"]}
            if "keys" in case:
                assert R.decode(by_kind[DATA], len(case["keys"]), False) == case["keys"], name
                assert R.decode(by_kind[LENGTH], len(case["dict_lengths"]), False) == case["dict_lengths"], name
            else:
                assert R.decode(by_kind[LENGTH], len(case["lengths"]), False) == case["lengths"], name


def test_model_and_oracle_agree_on_every_valid_direct_case():
    judge(VALID)


def test_model_and_oracle_agree_on_every_malformed_direct_case():
    judge(MALFORMED)


def test_model_and_oracle_agree_on_every_valid_dictionary_case():
    judge(DICT_VALID)


def test_model_and_oracle_agree_on_every_malformed_dictionary_case():
    judge(DICT_MALFORMED)


def test_a_binary_column_takes_what_a_string_column_refuses():
    """the same rows, the same streams: every UTF-8 failure of a String column is no failure of a Binary column"""
    n = 0
    for name, case in MALFORMED.items():
        if not name.startswith(("utf8/", "boundary/", "batch boundary/", "row boundary/", "ascii/")):
            continue
        n += 1
        for batch in case["batches"]:
            want = [(o, v, validity_want(case, batch)(b)) for b, (o, v) in enumerate(expect(case["rows"], batch))]
            assert M.direct(case["lengths"], case["present"], case["data"], batch, False) == (want, None), (name, batch)
            assert oracle_run(case, batch, dict(case["column"], orc_type=BINARY)) == (want, None), (name, batch)
    assert n >= 100


def test_char_and_varchar_decode_as_string():
    for table, names in ((VALID, ("utf8/F4 8F BF BF", "lengths/0 to 4097, with nulls")), (MALFORMED, ("utf8/ED A0 80", "sums/the sum is 2^31, batch 2")),
                         (DICT_VALID, ("an entry of 9 bytes, with nulls",)), (DICT_MALFORMED, ("dictionary/lengths 2^31 and -5", "keys/a key of 2^63"))):
        for name in names:
            case = table[name]
            for batch in case["batches"]:
                want = oracle_run(case, batch)
                for t in (VARCHAR, CHAR):
                    assert oracle_run(case, batch, dict(case["column"], orc_type=t)) == want, (name, t)


def test_there_are_no_string_vectors_of_the_reference_to_pass():
    """tests/kat_vectors.py holds the reference's own vectors: none of them is a string column (when one is added, the model
    has to pass it here)"""
    assert not [n for n in dir(K) if "STRING" in n or "UTF8" in n or "BINARY" in n]
