"""Hand-built Zstandard frames (tests/zstd_enc.py) and who accepts them.  The tables of this module are what
tests/test_gpu_zstd_frames.py pushes through the Zstandard kernels; here, without a GPU, every case is first shown to mean
what its name says.  A payload is one ORC chunk's bytes: one or more frames.

The judges: libzstd, reached through pyarrow's CompressedInputStream (it reads concatenated and skippable frames without being
told a size, as the reference's streaming decoder does), and the CPU oracle (oracle/oo_codecs.c, oo_zstd_frame).  The reference
decodes Zstandard WITH libzstd, so libzstd is the authority: a VALID case must come back as the writer's own model of the plain
bytes from both, a MALFORMED one must be refused by both, and the oracle gets no table of its own.  LIBZSTD_DIFFERS holds only
what is a limit of the ORC reader and not of the format: the output head-room of max(block size, 4 MiB).

Two sizes the format itself bounds: a block regenerates at most 128 KiB, so literals-length code 35 and match-length code 52
cannot take their highest extra bits (131069 literals and a match of 131072 are the most a block holds), and the highest LL, ML
and OF codes cannot meet in one sequence; the widest step here is LL code 34 + ML code 51 + OF code 18 with 9 + 9 + 8 state bits."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from zstd_enc import (BLOCK_MAX, LL_BASE, LL_BITS, MAGIC, ML_BASE, ML_BITS, PREDEF, REPEAT, Frame, Fse, HufLit, RawLit, Rep, Rle, RleLit, S, skippable)

pa = pytest.importorskip("pyarrow")

CAP = 1 << 22
_LANES_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orc_rust_amd", "csrc", "device", "zstd_lanes.h")
ZQ_STEPS = int(re.search(r"^#define ZQ_STEPS (\d+)", open(_LANES_H).read(), re.M).group(1))   # the step-group size of the lanes kernel

VALID = {}       # name -> (chunk payload, plain)
MALFORMED = {}   # name -> chunk payload
LIBZSTD_DIFFERS = {
    "output_beyond_the_head_room": "libzstd has no output limit: the max(block size, 4 MiB) a chunk may expand to is the ORC reader's",
}
# Damaged input that this libzstd happens to take, with bytes the format does not define: the oracle and the kernels follow RFC 8878
# and refuse.  name -> (payload, why).  Not a table of the issue's: nothing here is a frame a writer could mean.
RFC_FOLLOWED = {}


def payload_of(parts):
    return b"".join(p.finish() if isinstance(p, Frame) else bytes(p) for p in parts)


def valid(name, *parts):
    assert name not in VALID
    VALID[name] = (payload_of(parts), b"".join(p.plain() for p in parts if isinstance(p, Frame)))


def malformed(name, *parts):
    assert name not in MALFORMED and name not in VALID
    MALFORMED[name] = payload_of(parts)


def rnd(seed, n, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, n, dtype=np.uint8).tobytes()


def skewed(seed, n, scale=12.0, top=255):
    return np.minimum(top, np.random.default_rng(seed).exponential(scale, n).astype(np.int64)).astype(np.uint8).tobytes()


def some_seqs(seed, n, have, max_ll=5, max_ml=20, max_off=60):
    """n sequences that are valid behind `have` bytes, and the literals they need (plus three that stay behind the last match)."""
    rng = np.random.default_rng(seed)
    seqs, lits, matched = [], 0, 0
    for _ in range(n):
        ll = int(rng.integers(0, max_ll + 1)) if have + lits else int(rng.integers(1, max_ll + 1))
        ml = int(rng.integers(3, max_ml + 1))
        lits += ll
        seqs.append(S(ll, ml, int(rng.integers(1, min(have + lits + matched, max_off) + 1))))
        matched += ml
    return rnd(seed + 1000, lits + 3, 97, 123), seqs


def fresh(**kw):
    """A frame with a window descriptor (1 MiB) and a 4-byte content size.  A Single_Segment frame's window is its content size, and
    no Block_Size may exceed the window: small frames whose blocks do not compress could not be Single_Segment ones."""
    kw.setdefault("fcs_bytes", 4)
    kw.setdefault("single_segment", False)
    return Frame(**kw)


# ---- frame forms ---------------------------------------------------------------------------------------------------------------
valid("content_size_1_byte", Frame(fcs_bytes=1).raw(rnd(1, 200), last=True))
valid("content_size_2_bytes_256", Frame(fcs_bytes=2).raw(rnd(2, 256), last=True))
valid("content_size_2_bytes_65791", Frame(fcs_bytes=2).raw(rnd(3, 255)).rle(7, 65536, last=True))
valid("content_size_4_bytes", Frame(fcs_bytes=4).raw(rnd(4, 100), last=True))
valid("content_size_4_bytes_single_segment_compressed", Frame(fcs_bytes=4).compressed(*some_seqs(4, 30, 0), last=True))
valid("content_size_8_bytes", Frame(fcs_bytes=8).raw(rnd(5, 100), last=True))
valid("window_descriptor_with_content_size", Frame(fcs_bytes=4, single_segment=False).raw(rnd(6, 300), last=True))
valid("window_descriptor_without_content_size", Frame(fcs_bytes=0).raw(rnd(7, 300)).compressed(*some_seqs(8, 5, 300), last=True))
valid("checksum", Frame(fcs_bytes=2, checksum=True).raw(rnd(9, 300)).compressed(*some_seqs(10, 5, 300), last=True))
valid("checksum_without_content_size", Frame(fcs_bytes=0, checksum=True).rle(3, 77).raw(rnd(11, 30), last=True))
valid("skippable_in_front", skippable(b"skip me"), fresh().raw(b"behind a skippable frame", last=True))
valid("skippable_between", fresh().raw(b"one", last=True), skippable(b"", nibble=15), Frame(fcs_bytes=0).raw(b"two", last=True))
valid("skippable_behind", fresh().raw(b"in front of a skippable frame", last=True), skippable(rnd(12, 40), nibble=7))
valid("three_frames", Frame(fcs_bytes=1).compressed(*some_seqs(13, 4, 0), last=True), Frame(fcs_bytes=0).rle(9, 40, last=True),
      Frame(fcs_bytes=8, checksum=True).compressed(*some_seqs(14, 9, 0), last=True))
valid("empty_frame_between", fresh().raw(b"left", last=True), Frame(fcs_bytes=1).raw(b"", last=True), fresh().raw(b"right", last=True))
valid("empty_frame_first_and_last", Frame(fcs_bytes=1).raw(b"", last=True), fresh().raw(b"middle", last=True), Frame(fcs_bytes=1).raw(b"", last=True))
for _w in (1, 2, 4):
    valid("zero_dictionary_id_%d_bytes" % _w, Frame(fcs_bytes=1, dict_id=(_w, 0)).raw(b"no dictionary", last=True))


# ---- block mixes ---------------------------------------------------------------------------------------------------------------
def add_block(f, kind, seed, last=False):
    if kind == "raw":
        return f.raw(rnd(seed, 40), last=last)
    if kind == "rle":
        return f.rle(seed & 255, 40, last=last)
    return f.compressed(*some_seqs(seed, 6, len(f.out)), last=last)


for _a in ("raw", "rle", "compressed"):
    for _b in ("raw", "rle", "compressed"):
        _f = add_block(add_block(fresh(), _a, 20), _b, 21)
        # a third block whose matches reach into both
        valid("blocks_%s_then_%s" % (_a, _b), _f.compressed(RawLit(b"xy"), [S(1, 30, len(_f.out) - 5), S(0, 50, len(_f.out) + 1), S(1, 4, 45)], last=True))
valid("rle_block_of_1_byte", fresh().rle(0x5A, 1).compressed(RawLit(b""), [S(0, 9, 1)], last=True))
valid("rle_block_of_128_KiB", fresh().rle(0xA5, BLOCK_MAX).compressed(RawLit(b"q"), [S(1, 5, BLOCK_MAX + 1), S(0, 5, 3)], last=True))
valid("raw_block_of_128_KiB", fresh().raw(rnd(22, BLOCK_MAX), last=True))
valid("compressed_block_content_of_128_KiB", fresh().compressed(RawLit(rnd(23, BLOCK_MAX - 4), fmt=3), [], last=True))
assert len(VALID["compressed_block_content_of_128_KiB"][0]) == 4 + 2 + 4 + 3 + BLOCK_MAX
valid("compressed_block_regenerates_128_KiB_the_longest_match", fresh().raw(b"abc").compressed(RawLit(b""), [S(0, BLOCK_MAX, 3)], last=True))
valid("compressed_block_regenerates_128_KiB_literals_and_matches",
      fresh().compressed(RawLit(rnd(24, 1000)), [S(500, 65536, 77), S(499, BLOCK_MAX - 65536 - 1000, 499)], last=True))
assert len(VALID["compressed_block_regenerates_128_KiB_literals_and_matches"][1]) == BLOCK_MAX
valid("block_with_zero_sequences", fresh().compressed(RawLit(rnd(25, 50)), []).compressed(HufLit(skewed(26, 300), streams=1), [], last=True))
valid("block_with_zero_literals", fresh().raw(rnd(27, 64)).compressed(RawLit(b""), [S(0, 10, 64), S(0, 3, 1), S(0, 40, 20), Rep(0, 5, 1)], last=True))
valid("match_from_a_raw_block", fresh().raw(rnd(28, 100)).compressed(RawLit(b"z"), [S(1, 20, 90)], last=True))
valid("match_from_an_rle_block", fresh().raw(b"ab").rle(0x33, 100).compressed(RawLit(b"z"), [S(1, 20, 90), S(0, 7, 123)], last=True))
valid("match_from_a_compressed_block", fresh().compressed(*some_seqs(29, 8, 0)).compressed(RawLit(b"z"), [S(1, 20, 30)], last=True))
valid("match_reaches_the_first_byte_of_the_frame", fresh().raw(rnd(30, 77)).compressed(RawLit(b"zz"), [S(2, 10, 79), S(0, 89, 89)], last=True))
valid("match_reaches_the_first_byte_of_the_second_frame", fresh().raw(rnd(31, 50), last=True),
      fresh().compressed(RawLit(b"abcd"), [S(4, 10, 4), S(0, 3, 14)], last=True))

# ---- literals ------------------------------------------------------------------------------------------------------------------
for _fmt in (0, 1, 3):
    valid("raw_literals_size_format_%d" % _fmt, fresh().compressed(RawLit(rnd(40 + _fmt, 21), fmt=_fmt), [S(20, 5, 3)], last=True))
    valid("rle_literals_size_format_%d" % _fmt, fresh().raw(b"ab").compressed(RleLit(0x77, 20, fmt=_fmt), [S(7, 5, 8), S(12, 3, 1)], last=True))
valid("raw_literals_5_bits_31", fresh().compressed(RawLit(rnd(44, 31)), [S(31, 3, 31)], last=True))
valid("raw_literals_12_bits_4095", fresh().compressed(RawLit(rnd(45, 4095)), [S(4095, 3, 4095)], last=True))
valid("raw_literals_20_bits_4096", fresh().compressed(RawLit(rnd(46, 4096)), [S(4096, 3, 4096)], last=True))
valid("rle_literals_20_bits_128_KiB", fresh().compressed(RleLit(0x11, BLOCK_MAX), [], last=True))
valid("huffman_one_stream", fresh().compressed(HufLit(skewed(47, 700), streams=1), [S(300, 9, 200), S(398, 9, 7)], last=True))
for _fmt, _n in ((1, 900), (2, 900), (3, 900), (2, 5000), (3, 5000), (3, 40000)):
    valid("huffman_four_streams_size_format_%d_%d_literals" % (_fmt, _n), fresh().compressed(HufLit(skewed(48 + _fmt, _n), fmt=_fmt), [S(100, 30, 50)], last=True))
for _n in (6, 7, 8, 9, 10, 11, 400, 401, 402, 403):
    valid("huffman_four_streams_%d_literals" % _n, fresh().compressed(HufLit(skewed(60, _n, 3.0), fmt=1), [S(_n - 1, 4, 2)], last=True))
valid("huffman_two_symbols", fresh().compressed(HufLit(rnd(61, 300, 0, 2), streams=1, weights=[1, 1]), [S(299, 3, 1)], last=True))
valid("huffman_two_symbols_far_apart", fresh().compressed(HufLit(bytes(b * 100 for b in rnd(62, 200, 0, 2)), weights=[1] + [0] * 99 + [1]), [], last=True))
_w256 = [9] + [2] + [1] * 254   # symbol 0: 1 bit, symbol 1: 8 bits, the others 9; the weight of symbol 255 is implied
valid("huffman_256_symbols", fresh().compressed(HufLit(bytes(range(256)) * 2 + rnd(63, 600) + bytes([255, 0, 255]), weights=_w256, desc="fse"), [S(700, 50, 256)], last=True))
_w11 = [11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1]   # code lengths 1, 2, .., 10, 11, 11
valid("huffman_11_bit_codes", fresh().compressed(HufLit(skewed(64, 500, 1.5, 11) + bytes(range(12)) + bytes([11, 10, 11]), streams=1, weights=_w11), [], last=True))
valid("huffman_11_bit_codes_four_streams", fresh().compressed(HufLit(rnd(65, 3000, 0, 12), weights=_w11), [S(1500, 5, 3)], last=True))
_wgap = [3, 0, 0, 2, 0, 1, 0, 0, 0, 0, 1]          # absent symbols in the middle
valid("huffman_absent_symbols", fresh().compressed(HufLit(bytes([0, 3, 5, 10][b] for b in rnd(66, 400, 0, 4)), weights=_wgap), [], last=True))
valid("huffman_direct_weights_odd_count", fresh().compressed(HufLit(rnd(67, 200, 0, 4), weights=[3, 1, 1, 2], streams=1), [], last=True))
valid("huffman_direct_weights_even_count", fresh().compressed(HufLit(rnd(68, 200, 0, 5), weights=[2, 2, 1, 1, 2], streams=1), [], last=True))
valid("huffman_direct_weights_128", fresh().compressed(HufLit(bytes([0, 5, 128][b] for b in rnd(69, 200, 0, 3)), weights=[1] + [0] * 4 + [1] + [0] * 122 + [2], streams=1, desc="direct"), [], last=True))
valid("huffman_fse_weights_of_few_symbols", fresh().compressed(HufLit(rnd(70, 300, 0, 12), weights=_w11, desc="fse", fse_log=5), [], last=True))
valid("huffman_fse_weights_log_6", fresh().compressed(HufLit(skewed(71, 2000, 20.0, 200)), [S(1000, 100, 500)], last=True))


def treeless_chain(between):
    f = fresh().compressed(HufLit(skewed(72, 600, 4.0, 30) + bytes(range(31))), [S(100, 8, 50)])
    between(f)
    return f.compressed(HufLit(skewed(73, 500, 4.0, 30)[:333], treeless=True), [S(5, 8, 50)], last=True)


valid("treeless_right_behind_its_tree", treeless_chain(lambda f: None))
valid("treeless_behind_a_raw_block", treeless_chain(lambda f: f.raw(rnd(74, 33))))
valid("treeless_behind_an_rle_block", treeless_chain(lambda f: f.rle(1, 33)))
valid("treeless_behind_raw_literals", treeless_chain(lambda f: f.compressed(RawLit(rnd(75, 33)), [S(3, 3, 3)])))
valid("treeless_behind_rle_literals_and_an_empty_block", treeless_chain(lambda f: f.compressed(RleLit(9, 33), []).raw(b"")))
valid("treeless_size_format_2", treeless_chain(lambda f: f.compressed(HufLit(skewed(78, 5000, 4.0, 30), fmt=2, treeless=True), [])))
valid("treeless_size_format_3", treeless_chain(lambda f: f.compressed(HufLit(skewed(79, 5000, 4.0, 30), fmt=3, treeless=True), [S(2000, 3000, 1500)])))
valid("treeless_twice_in_a_row", treeless_chain(lambda f: f.compressed(HufLit(skewed(76, 40, 4.0, 30), streams=1, treeless=True), [])))
valid("treeless_one_stream_several_blocks_back", treeless_chain(lambda f: f.raw(b"a").rle(2, 2).compressed(RawLit(b"b"), []).compressed(HufLit(skewed(77, 90, 4.0, 30), streams=1, treeless=True), [])))

# ---- sequence tables -----------------------------------------------------------------------------------------------------------
_same = [S(2, 7, 5)] * 6   # one code in every table: RLE_Mode can carry it
MODES = {"predefined": lambda: PREDEF, "rle": lambda: Rle(), "fse": lambda: Fse(log=6), "repeat": lambda: REPEAT}
for _pos in ("ll", "of", "ml"):
    for _mode in MODES:
        _f = fresh().raw(rnd(79, 8)).compressed(RawLit(rnd(80, 14)), _same)   # (three predefined tables for a Repeat_Mode to repeat)
        valid("mode_%s_in_%s" % (_mode, _pos), _f.compressed(RawLit(rnd(81, 14)), _same, last=True, **{_pos: MODES[_mode]()}))
_l, _s = some_seqs(82, 40, 0)
_l2, _s2 = some_seqs(83, 25, 500)


def repeat_case(first, between=lambda f: None):
    # (the repeating block's codes must be among the first one's: the first block holds its sequences too)
    f = fresh().raw(rnd(84, 500)).compressed(RawLit(_l[:-3] + _l2), _s + _s2 if first != "rle" else _same * 8, **{k: first_mode(first) for k in ("ll", "of", "ml")})
    between(f)
    return f.compressed(RawLit(_l2), _s2 if first != "rle" else _same * 3, ll=REPEAT, of=REPEAT, ml=REPEAT, last=True)


def first_mode(kind):
    return {"fse": Fse(log=7), "rle": Rle(), "predefined": PREDEF}[kind]


for _kind in ("fse", "rle", "predefined"):
    valid("repeat_of_%s_tables" % _kind, repeat_case(_kind))
valid("repeat_across_a_block_without_sequences", repeat_case("fse", lambda f: f.compressed(RawLit(b"no sequences"), [])))
valid("repeat_across_a_raw_block_and_an_rle_block", repeat_case("fse", lambda f: f.raw(b"raw").rle(0, 9)))
valid("repeat_of_a_repeat", repeat_case("fse", lambda f: f.compressed(RawLit(_l2), _s2, ll=REPEAT, of=REPEAT, ml=REPEAT)))
valid("repeat_of_one_table_only", fresh().raw(rnd(85, 500)).compressed(RawLit(_l[:-3] + _l2), _s + _s2, of=Fse(log=6)).compressed(RawLit(_l2), _s2, ll=Fse(log=5), of=REPEAT, last=True))
for _name, _logs in (("lowest", (5, 5, 5)), ("highest", (9, 8, 9))):
    valid("accuracy_logs_%s" % _name, fresh().raw(rnd(86, 500)).compressed(RawLit(_l), _s, ll=Fse(log=_logs[0]), of=Fse(log=_logs[1]), ml=Fse(log=_logs[2]), last=True))
# "less than 1" probabilities: the rare codes of each table
_rare = [S(1, 3, 1)] * 20 + [S(30, 100, 200), S(1, 3, 1), S(17, 40, 1000), S(1, 3, 1)] + [S(2, 4, 2)] * 10
valid("less_than_1_probabilities", fresh().raw(rnd(87, 1000)).compressed(
    RawLit(rnd(88, 200)), _rare, ll=Fse(log=6, low=(21, 16)), of=Fse(log=5, low=(7, 9)), ml=Fse(log=6, low=(42, 34)), last=True))
# zero runs: the repeat flags 0, 1, 2 and a chain of 3s (3, 3, 1); every table ends in the middle of a byte or not as its counts fall
_zr_ll = [S(ll, 3, 1) for ll in (0, 2, 5, 9, 19)] * 3     # LL codes 0, 2 (flag 0), 5 (flag 1), 9 (flag 2), 17 (3, 3, 1)
_zr_ml = [S(0, ml, 1) for ml in (3, 5, 8, 12, 22)] * 3    # ML codes 0, 2, 5, 9, 19: the same, and 3, 3, 2
valid("zero_runs_with_every_repeat_flag", fresh().raw(b"r").compressed(RawLit(rnd(89, 200)), _zr_ll + _zr_ml, ll=Fse(log=5), ml=Fse(log=6), of=Fse(log=5), last=True))
valid("zero_run_chain_of_3s_up_to_the_last_code", fresh().raw(rnd(90, 70000)).compressed(
    RawLit(rnd(91, 70000)), [S(0, 3, 1)] * 3 + [S(65536, 3, 1), S(0, 65539 - 20000, 60000)], ll=Fse(log=5), ml=Fse(log=5), of=Fse(log=5), last=True))

# ---- codes and bits ------------------------------------------------------------------------------------------------------------
def pack(f, seqs, seed, lit=RawLit, **kw):
    """The sequences in as few blocks as the 128 KiB a block regenerates allow, raw literals; the last one closes the frame."""
    blocks, cur, size = [], [], 0
    for q in seqs:
        if size + q.ll + q.ml > BLOCK_MAX:
            blocks.append(cur)
            cur, size = [], 0
        cur.append(q)
        size += q.ll + q.ml
    blocks.append(cur)
    for k, b in enumerate(blocks):
        n = sum(q.ll for q in b)
        f.compressed(lit(rnd(seed + k, n) if lit is RawLit else skewed(seed + k, n, 6.0, 60)), b, last=k + 1 == len(blocks), **kw)
    return f


def length_ends(base, bits, codes, most):
    return [min(v, most) for c in codes for v in (base[c], base[c] + (1 << bits[c]) - 1)]


valid("literals_length_codes_0_to_31", pack(fresh().raw(b"0123456789abcdef"), [S(ll, 3 + k % 5, 1 + k % 16) for k, ll in enumerate(length_ends(LL_BASE, LL_BITS, range(32), 1 << 20))], 100))
valid("literals_length_codes_32_to_34", pack(fresh().raw(b"0123456789abcdef"), [S(ll, 3 + k % 5, 1 + k % 16) for k, ll in enumerate(length_ends(LL_BASE, LL_BITS, range(32, 35), 1 << 20))], 110))
valid("literals_length_code_35", pack(fresh().raw(b"0123456789abcdef"), [S(ll, 3, 16) for ll in length_ends(LL_BASE, LL_BITS, [35], BLOCK_MAX - 3)], 120, lit=HufLit))   # (raw, the block's content would be above 128 KiB)
valid("match_length_codes_0_to_50", pack(fresh().raw(b"0123456789abcdef"), [S(k % 3, ml, 1 + k % 16) for k, ml in enumerate(length_ends(ML_BASE, ML_BITS, range(51), 1 << 20))], 130))
valid("match_length_codes_51_and_52", pack(fresh().raw(b"0123456789abcdef"), [S(0, ml, 1 + k % 16) for k, ml in enumerate(length_ends(ML_BASE, ML_BITS, [51, 52], BLOCK_MAX))], 140))
# offset codes: the value is offset + 3, code c covers the values 2^c .. 2^(c+1) - 1; 262152 bytes in front reach the lowest value of code 18
_far = fresh().raw(rnd(150, BLOCK_MAX)).raw(rnd(151, BLOCK_MAX)).raw(b"8 more..")
_offs = [v - 3 for c in range(2, 18) for v in (1 << c, (2 << c) - 1)] + [(1 << 18) - 3]
valid("offset_codes_2_to_18", _far.compressed(RawLit(rnd(152, 40)), [S(1, 3 + k % 4, o) for k, o in enumerate(_offs)], last=True))
valid("offset_codes_2_to_18_fse_table", fresh().raw(rnd(153, BLOCK_MAX)).raw(rnd(154, BLOCK_MAX)).raw(b"8 more..").compressed(
    RawLit(rnd(155, 40)), [S(1, 3 + k % 4, o) for k, o in enumerate(_offs)], of=Fse(log=8), last=True))
# the widest step: 18 + 15 + 15 extra bits and 9 + 9 + 8 state bits ("less than 1" symbols take a whole accuracy log)
_wide = fresh().raw(rnd(156, BLOCK_MAX)).raw(rnd(157, 68000))
_wseq = [S(1, 3, 1)] * 20 + [S(65535, 40000, (1 << 18) + 2000 - 3), S(1, 3, 1)] + [S(2, 4, 2)] * 5
_wide.compressed(RawLit(rnd(159, 65600)), _wseq, ll=Fse(log=9, low=(34,)), of=Fse(log=8, low=(18,)), ml=Fse(log=9, low=(51,)), last=True, widest=True)
assert _wide.step_bits == 18 + 15 + 15 + 9 + 9 + 8, _wide.step_bits
valid("widest_step_74_bits", _wide)
for _n, _form in ((1, None), (127, None), (128, None), (0x7EFF, None), (0x7F00, None), (5, 2), (127, 2), (300, 2)):
    _l3, _s3 = some_seqs(160 + _n, _n, 0, max_ll=1, max_ml=3)
    valid("number_of_sequences_%d%s" % (_n, "_in_2_bytes" if _form else ""), fresh().compressed(RawLit(_l3), _s3, nseq_form=_form, last=True))
# the final-bit marker: one sequence, three RLE tables, offset code c: c bits of stream
for _c in range(2, 10):
    valid("final_bit_marker_behind_%d_bits" % _c, fresh().raw(rnd(170, 1024)).compressed(RawLit(b"m"), [S(1, 4, (1 << _c) + _c - 3)], ll=Rle(), of=Rle(), ml=Rle(), last=True))
assert {VALID["final_bit_marker_behind_%d_bits" % c][0][-1].bit_length() for c in range(2, 10)} == set(range(1, 9))

# ---- repeat offsets ------------------------------------------------------------------------------------------------------------
# three RLE tables per block, so that the coverage test can read the codes back without an FSE decoder
_rep = fresh().raw(rnd(180, 100)).compressed(RawLit(b"abcdef"), [S(2, 4, 30), S(2, 4, 50), S(2, 4, 70)], of=Fse(log=5))
for _code in (1, 2, 3):
    for _ll in (2, 0):
        _rep.compressed(RawLit(rnd(181, 2 * _ll)), [Rep(_ll, 5, _code)] * 2, ll=Rle(), of=Rle(), ml=Rle())
valid("repeat_codes_with_and_without_literals", _rep.raw(b"", last=True))
valid("start_of_frame_history_1_4_8", fresh().compressed(RawLit(rnd(182, 12)), [Rep(9, 3, 3), Rep(1, 3, 3), Rep(1, 4, 2), Rep(1, 5, 1)], last=True))
valid("start_of_frame_history_behind_a_raw_block", fresh().raw(rnd(183, 8)).compressed(RawLit(b""), [Rep(0, 3, 2), Rep(0, 3, 1), Rep(0, 3, 2)], last=True))
valid("repeat_1_minus_1", fresh().raw(rnd(184, 40)).compressed(RawLit(b"k"), [S(1, 3, 20), Rep(0, 4, 3), Rep(0, 4, 3), Rep(0, 5, 1), Rep(0, 5, 2)], last=True))
valid("history_across_compressed_blocks", fresh().raw(rnd(185, 99)).compressed(RawLit(b"abc"), [S(1, 3, 11), S(1, 3, 22), S(1, 3, 33)]).compressed(
    RawLit(b"de"), [Rep(1, 4, 3), Rep(0, 4, 2)]).compressed(RawLit(b"f"), [Rep(0, 3, 3), Rep(1, 3, 1), Rep(0, 6, 1)], last=True))
valid("history_across_raw_rle_and_empty_blocks", fresh().raw(rnd(186, 99)).compressed(RawLit(b"abc"), [S(1, 3, 11), S(1, 3, 22), S(1, 3, 33)]).raw(b"raw").compressed(
    RawLit(b"de"), [Rep(1, 4, 3)]).rle(4, 4).compressed(RawLit(b"none"), []).compressed(RawLit(b"f"), [Rep(0, 3, 2), Rep(1, 3, 2), Rep(0, 6, 1)], last=True))
valid("history_starts_again_in_the_next_frame", fresh().raw(rnd(187, 30)).compressed(RawLit(b"a"), [S(1, 3, 25)], last=True),
      fresh().raw(rnd(188, 30)).compressed(RawLit(b"b"), [Rep(1, 3, 1), Rep(0, 3, 2), Rep(0, 3, 3)], last=True))

# ---- copies --------------------------------------------------------------------------------------------------------------------
valid("offsets_1_to_16_overlapping", fresh().raw(rnd(190, 16)).compressed(RawLit(rnd(191, 16)), [S(1, 40 * o + o // 2, o) for o in range(1, 17)], last=True))
valid("offsets_1_to_16_overlapping_no_literals", fresh().raw(rnd(192, 16)).compressed(RawLit(b""), [S(0, 300 + 7 * o, o) for o in range(1, 17)], last=True))

# ---- lane boundaries -----------------------------------------------------------------------------------------------------------
for _n in (1, 2, 3, 4, 5, 7, 8, 9, ZQ_STEPS - 1, ZQ_STEPS, ZQ_STEPS + 1, 3 * ZQ_STEPS - 1, 3 * ZQ_STEPS, 3 * ZQ_STEPS + 1):
    _l4, _s4 = some_seqs(200 + _n, _n, 64)
    valid("block_of_%d_sequences" % _n, fresh().raw(rnd(201, 64)).compressed(HufLit(_l4, streams=1), _s4, ll=Fse(log=6), of=Fse(log=5), ml=Fse(log=6), last=True))
_f = fresh().raw(rnd(202, 64))
for _n in (ZQ_STEPS + 1, 1, ZQ_STEPS, 2, 5 * ZQ_STEPS - 1):
    _f.compressed(*some_seqs(210 + _n, _n, 64))
valid("blocks_of_many_lengths_in_one_frame", _f.raw(b"", last=True))

assert all(len(p) <= 300 * 1024 for _, p in VALID.values()), [(n, len(p)) for n, (_, p) in VALID.items() if len(p) > 300 * 1024]


# ---- malformed -----------------------------------------------------------------------------------------------------------------
def bad(**kw):
    kw.setdefault("fcs_bytes", 4)
    kw.setdefault("single_segment", kw["fcs_bytes"] == 0 and None)
    return Frame(check=False, **kw)


_good = lambda: fresh().raw(b"a good frame", last=True)
malformed("bad_magic", b"\x28\xb5\x2f\xfc" + _good().finish()[4:])
malformed("bad_magic_behind_a_frame", _good(), b"\x27\xb5\x2f\xfd" + _good().finish()[4:])
malformed("reserved_frame_header_bit", Frame(fcs_bytes=1, reserved=True).raw(b"reserved", last=True))
for _w in (1, 2, 4):
    malformed("dictionary_id_%d_bytes" % _w, Frame(fcs_bytes=1, dict_id=(_w, 1 << (8 * _w - 1))).raw(b"a dictionary", last=True))
# Block_Maximum_Size is the smaller of the window and 128 KiB: window descriptor 0 is 1 KiB, 1 is 1 KiB + 1/8
valid("blocks_of_exactly_the_window", Frame(fcs_bytes=0, window=1).raw(rnd(215, 1152)).rle(3, 1152).compressed(RawLit(b"ab"), [S(2, 1150, 7)], last=True))
malformed("raw_block_above_the_window", Frame(fcs_bytes=0, window=0).raw(rnd(216, 1025), last=True))
malformed("rle_block_above_the_window", Frame(fcs_bytes=0, window=0).rle(5, 1025, last=True))
malformed("compressed_block_above_the_window", bad(fcs_bytes=0, window=0).raw(b"abc").compressed(RawLit(rnd(217, 1023)), [], last=True))
malformed("block_regenerates_more_than_the_window", bad(fcs_bytes=0, window=0).raw(b"abc").compressed(RawLit(b"d"), [S(1, 1024, 3)], last=True))
malformed("compressed_block_above_the_content_size", Frame(fcs_bytes=1, check=False).compressed(RawLit(b"abcdefgh"), [S(8, 5, 3)], last=True))
malformed("raw_block_above_128_KiB", Frame(fcs_bytes=0).raw(rnd(220, BLOCK_MAX + 1), last=True))
malformed("rle_block_above_128_KiB", Frame(fcs_bytes=0).rle(0x21, BLOCK_MAX + 1, last=True))
malformed("compressed_block_above_128_KiB", bad().compressed(RawLit(rnd(221, BLOCK_MAX - 3), fmt=3), [], last=True))
malformed("reserved_block_type", fresh().raw(b"ok").reserved_block(b"what", last=True))
malformed("no_last_block", fresh().raw(b"there is no last block"))
malformed("no_last_block_behind_a_compressed_block", fresh().compressed(*some_seqs(222, 4, 0)))
malformed("skippable_frame_cut", _good(), skippable(b"12345678")[:-3])
malformed("skippable_frame_header_cut", _good(), skippable(b"")[:6])


# truncation: a frame with every header field and every section, cut inside each
def sweep_frame():
    f = Frame(fcs_bytes=4, single_segment=False, dict_id=(2, 0), checksum=True)
    f.compressed(HufLit(skewed(223, 600, 4.0, 40)), some_seqs(224, 30, 0, max_ll=15)[1], ll=Fse(log=6), of=Fse(log=5), ml=Fse(log=6), last=True)
    return f


_sw = sweep_frame()
SWEEP = _sw.finish()
valid("the_frame_of_the_truncation_sweep", _sw)
_hdr = len(_sw.header())
# every byte of the frame header, the block header and the literals header; then places spread over tree, streams, tables and bits
_cuts = set(range(1, _hdr + 3 + 4 + 1)) | {_hdr + 7 + (k * (len(SWEEP) - 5 - _hdr - 7)) // 11 for k in range(1, 12)} | {len(SWEEP) - 5, len(SWEEP) - 4, len(SWEEP) - 1}
for _c in sorted(_cuts):
    malformed("cut_at_byte_%03d" % _c, SWEEP[:_c])

# literals and Huffman
malformed("treeless_without_a_tree", bad().raw(b"raw").compressed(HufLit(skewed(225, 100, 4.0, 30), streams=1, treeless=True), [], last=True))
malformed("treeless_with_a_tree_in_the_frame_before_only", fresh().compressed(HufLit(skewed(226, 100, 4.0, 30), streams=1), [], last=True),
          bad().compressed(HufLit(skewed(226, 100, 4.0, 30), streams=1, treeless=True), [], last=True))


def poke(section, fn):
    return lambda name, b: fn(bytearray(b)) if name == section else b


def _set(i, v):
    def f(b):
        b[i] = v
        return bytes(b)
    return f


malformed("raw_literals_size_beyond_the_block", bad().compressed(RawLit(rnd(227, 40)), [], last=True, tamper=poke("literals", lambda b: bytes([1 << 2 | (200 & 15) << 4, 200 >> 4]) + bytes(b[2:]))))
malformed("huffman_compressed_size_beyond_the_block", bad().compressed(HufLit(skewed(228, 300, 4.0, 30), streams=1), [], last=True,
                                                                          tamper=poke("literals", lambda b: (int.from_bytes(b[:3], "little") + (40 << 14)).to_bytes(3, "little") + bytes(b[3:]))))


def jump_table_too_large(b):
    # (the tree's description: a header byte, then as many bytes as it says, or (n + 1) / 2 for direct weights)
    tree = 1 + (b[3] if b[3] < 128 else (b[3] - 127 + 1) // 2)
    b[3 + tree + 4:3 + tree + 6] = (0x3FF).to_bytes(2, "little")
    return bytes(b)


malformed("jump_table_beyond_the_section", bad().compressed(HufLit(skewed(229, 300, 4.0, 30), fmt=1), [], last=True, tamper=poke("literals", jump_table_too_large)))
malformed("huffman_weights_not_a_power_of_two", bad().compressed(RawLit(b""), [], last=True, tamper=poke(
    "literals", lambda b: (2 | 0 << 2 | 10 << 4 | 7 << 14).to_bytes(3, "little") + bytes([127 + 3, 0x22, 0x10]) + b"\x01\x01\x01\x01")))
_w12 = [12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1]   # code lengths 1 .. 11, 12, 12
# libzstd takes codes of 12 bits (its HUF_TABLELOG_MAX), one more than RFC 8878 4.2.1 allows: the authority says VALID, and 13 is refused
valid("huffman_12_bit_codes", fresh().compressed(HufLit(rnd(230, 300, 0, 13), streams=1, weights=_w12), [S(100, 9, 50)], last=True))
valid("huffman_12_bit_codes_four_streams", fresh().compressed(HufLit(rnd(231, 3001, 0, 13), weights=_w12), [S(1500, 5, 3)]).compressed(
    HufLit(rnd(232, 77, 0, 13), streams=1, treeless=True), [], last=True))
valid("huffman_12_bit_codes_weight_12_fse", fresh().compressed(HufLit(rnd(233, 300, 0, 13), streams=1, weights=_w12, desc="fse", fse_log=5), [], last=True))
malformed("huffman_13_bit_codes", bad().compressed(HufLit(rnd(234, 300, 0, 14), streams=1, weights=[13] + _w12), [], last=True))
malformed("huffman_12_bit_stream_ends_early", bad(fcs_bytes=0).compressed(HufLit(rnd(235, 300, 0, 13), streams=1, weights=_w12), [], last=True,
                                                                 tamper=poke("literals", lambda b: (int.from_bytes(b[:3], "little") + (1 << 4)).to_bytes(3, "little") + bytes(b[3:]))))
malformed("huffman_12_bit_stream_ends_late", bad(fcs_bytes=0).compressed(HufLit(rnd(235, 300, 0, 13), streams=1, weights=_w12), [], last=True,
                                                                tamper=poke("literals", lambda b: (int.from_bytes(b[:3], "little") - (1 << 4)).to_bytes(3, "little") + bytes(b[3:]))))
malformed("huffman_stream_ends_early", bad(fcs_bytes=0).compressed(HufLit(skewed(231, 300, 4.0, 30), streams=1), [], last=True,
                                                          tamper=poke("literals", lambda b: (int.from_bytes(b[:3], "little") + (1 << 4)).to_bytes(3, "little") + bytes(b[3:]))))
malformed("huffman_stream_ends_late", bad(fcs_bytes=0).compressed(HufLit(skewed(231, 300, 4.0, 30), streams=1), [], last=True,
                                                         tamper=poke("literals", lambda b: (int.from_bytes(b[:3], "little") - (1 << 4)).to_bytes(3, "little") + bytes(b[3:]))))
malformed("huffman_stream_without_a_marker", bad().compressed(HufLit(skewed(232, 300, 4.0, 30), streams=1), [], last=True, tamper=poke("literals", _set(-1, 0))))
# each of the first three streams of four is asked for one symbol more than it holds: libzstd's four-stream decoder does not notice
_early = bad(fcs_bytes=0).compressed(HufLit(skewed(233, 403, 4.0, 30), fmt=1), [], last=True,
                                     tamper=poke("literals", lambda b: (int.from_bytes(b[:3], "little") + (4 << 4)).to_bytes(3, "little") + bytes(b[3:])))
RFC_FOLLOWED["huffman_three_of_four_streams_end_early"] = (_early.finish(), "libzstd checks the four streams' ends loosely; RFC 8878 4.2.2: a stream must be used up exactly")

# sequence tables
_sl, _ss = some_seqs(234, 12, 0)
malformed("repeat_mode_without_a_table", bad().compressed(RawLit(_sl), _ss, ll=REPEAT, last=True))
malformed("repeat_mode_with_tables_in_the_frame_before_only", fresh().compressed(RawLit(_sl), _ss, last=True), bad().compressed(RawLit(_sl), _ss, of=REPEAT, last=True))
malformed("modes_byte_reserved_bits", fresh().compressed(RawLit(_sl), _ss, last=True, modes_reserved=1))
malformed("modes_byte_reserved_bits_2", fresh().compressed(RawLit(_sl), _ss, last=True, modes_reserved=2))
# an FSE description whose counts are not complete when the block ends: the table bytes are cut and the bit stream dropped
malformed("fse_description_overruns_the_block", fresh().compressed(RawLit(_sl), _ss, ml=Fse(log=6), last=True, tamper=lambda n, b: b[:2] if n == "tables" else b"" if n == "bits" else b))
malformed("fse_accuracy_log_too_high_ll", fresh().compressed(RawLit(_sl), _ss, ll=Fse(log=10), last=True))
malformed("fse_accuracy_log_too_high_of", fresh().compressed(RawLit(_sl), _ss, of=Fse(log=9), last=True))
malformed("fse_accuracy_log_too_high_ml", fresh().compressed(RawLit(_sl), _ss, ml=Fse(log=10), last=True))
# symbols beyond the tables' maxima: LL 36, ML 53, OF 32 (no sequence uses them; the description is the error)
malformed("fse_symbol_beyond_the_maximum_ll", fresh().compressed(RawLit(b"abc"), [S(1, 3, 1)] * 3, ll=Fse(norm=[0, 31] + [0] * 34 + [1], log=5), last=True))
malformed("fse_symbol_beyond_the_maximum_ml", fresh().compressed(RawLit(b"abc"), [S(1, 3, 1)] * 3, ml=Fse(norm=[31] + [0] * 52 + [1], log=5), last=True))
malformed("fse_symbol_beyond_the_maximum_of", fresh().compressed(RawLit(b"abc"), [S(1, 3, 1)] * 3, of=Fse(norm=[0, 0, 31] + [0] * 29 + [1], log=5), last=True))
malformed("rle_symbol_beyond_the_maximum_ll", bad().compressed(RawLit(b"abc"), [S(1, 3, 1)] * 3, ll=Rle(36), last=True))
malformed("rle_symbol_beyond_the_maximum_ml", bad().compressed(RawLit(b"abc"), [S(1, 3, 1)] * 3, ml=Rle(53), last=True))
malformed("rle_symbol_beyond_the_maximum_of", bad().compressed(RawLit(b"abc"), [S(1, 3, 1)] * 3, of=Rle(32), last=True))

# the sequences bit stream
malformed("sequences_stream_without_a_marker", fresh().compressed(RawLit(_sl), _ss, last=True, tamper=poke("bits", lambda b: bytes(b) + b"\x00")))
malformed("sequences_stream_bits_left_over", fresh().compressed(RawLit(_sl), _ss, last=True, tamper=poke("bits", lambda b: b"\x5a" + bytes(b))))
malformed("sequences_stream_bits_missing", fresh().compressed(RawLit(_sl), _ss, last=True, tamper=poke("bits", lambda b: bytes(b[1:]))))
malformed("sequences_stream_one_sequence_too_many", bad(fcs_bytes=0).compressed(RawLit(_sl), _ss, last=True, nseq=len(_ss) + 1))
malformed("sequences_stream_one_sequence_too_few", bad(fcs_bytes=0).compressed(RawLit(_sl), _ss, last=True, nseq=len(_ss) - 1))
malformed("sequences_stream_missing", fresh().compressed(RawLit(_sl), _ss, last=True, tamper=poke("bits", lambda b: b"")))

# sequence execution
malformed("literal_lengths_above_the_literals", bad().compressed(RawLit(b"abcd"), [S(2, 3, 1), S(3, 3, 1)], last=True))
malformed("offset_before_the_start_of_the_frame", bad().raw(b"abcde").compressed(RawLit(b"f"), [S(1, 3, 7)], last=True))
malformed("offset_before_the_start_of_the_second_frame", _good(), bad().compressed(RawLit(b"f"), [S(1, 3, 2)], last=True))
malformed("repeat_offset_in_an_empty_frame", bad().compressed(RawLit(b""), [Rep(0, 3, 1)], last=True))
malformed("offset_zero_through_repeat_1_minus_1", bad().raw(b"abcde").compressed(RawLit(b""), [S(0, 3, 1), Rep(0, 3, 3)], last=True))
malformed("block_regenerates_more_than_128_KiB", bad(fcs_bytes=0).raw(b"abc").compressed(RawLit(b"d"), [S(1, BLOCK_MAX, 3)], last=True))
malformed("block_regenerates_more_than_128_KiB_by_literals_left_over", bad(fcs_bytes=0).raw(b"abc").compressed(RawLit(b"de"), [S(1, BLOCK_MAX - 1, 3)], last=True))

# totals
malformed("content_shorter_than_stated", Frame(fcs_bytes=4, fcs=13).raw(b"twelve bytes", last=True))
malformed("content_longer_than_stated", Frame(fcs_bytes=4, fcs=11).raw(b"twelve bytes", last=True))
malformed("content_longer_than_stated_compressed", Frame(fcs_bytes=1, fcs=20).compressed(RawLit(b"ab"), [S(2, 19, 1)], last=True))
malformed("wrong_checksum", Frame(fcs_bytes=4, checksum="wrong").raw(b"the checksum is off by a bit", last=True))
malformed("wrong_checksum_of_the_second_frame", Frame(fcs_bytes=4, checksum=True).raw(b"right", last=True), Frame(fcs_bytes=0, checksum="wrong").rle(1, 100, last=True))
_big = Frame(fcs_bytes=0)
for _k in range(CAP // BLOCK_MAX):
    _big.rle(_k, BLOCK_MAX)
malformed("output_beyond_the_head_room", _big.rle(0xFF, 1, last=True))
assert len(_big.plain()) == CAP + 1


# ---- the judges ----------------------------------------------------------------------------------------------------------------
def libzstd(payload):
    """(plain, None) when libzstd's streaming decoder takes the payload to its end, else (None, why)."""
    try:
        return pa.CompressedInputStream(pa.BufferReader(payload), "zstd").read(), None
    except Exception as e:   # (pyarrow raises OSError or ArrowInvalid, by version)
        return None, str(e)


def oracle(payload, cap=CAP):
    return O.codec("zstd", payload, cap)


@pytest.mark.parametrize("name", list(VALID))
def test_valid_case_is_accepted_by_libzstd_and_the_oracle(name):
    payload, plain = VALID[name]
    got, why = libzstd(payload)
    assert got is not None, (name, "libzstd refuses it", why)
    assert got == plain, (name, "libzstd differs from the model", len(got), len(plain))
    o = oracle(payload)
    assert o is not None, (name, "the oracle rejects it")
    assert o == plain, (name, "the oracle differs from the model", len(o), len(plain))
    if len(plain):
        assert oracle(payload, len(plain)) == plain, (name, "a slot of exactly the plain size")
        assert oracle(payload, len(plain) - 1) is None, (name, "a slot one byte short")


@pytest.mark.parametrize("name", list(MALFORMED))
def test_malformed_case_is_rejected_by_libzstd_and_the_oracle(name):
    payload = MALFORMED[name]
    got, why = libzstd(payload)
    if name not in LIBZSTD_DIFFERS:
        assert got is None, (name, "libzstd accepts it", len(got))
    else:
        assert got is not None, (name, "libzstd agrees after all: take it out of LIBZSTD_DIFFERS", why)
    assert oracle(payload) is None, (name, "the oracle accepts it")


@pytest.mark.parametrize("name", list(RFC_FOLLOWED))
def test_damaged_input_libzstd_happens_to_take_is_refused(name):
    payload, why = RFC_FOLLOWED[name]
    assert why and oracle(payload) is None, (name, "the oracle accepts it")
    print(name, "libzstd:", "takes it" if libzstd(payload)[0] is not None else "refuses it too: move the case to MALFORMED")


def test_the_tables_are_what_the_issue_asks_for():
    assert len(VALID) >= 150 and len(MALFORMED) >= 60
    assert set(LIBZSTD_DIFFERS) <= set(MALFORMED) and all(LIBZSTD_DIFFERS.values())
    assert set(LIBZSTD_DIFFERS) == {"output_beyond_the_head_room"}   # capacity cases only
    assert sum(1 for n in MALFORMED if n.startswith("cut_at_byte_")) >= 25


# ---- were the forms really produced? -------------------------------------------------------------------------------------------
def walk(payload, seen):
    """The headers of a valid payload, read back in a few lines: what is found is added to `seen`.  Blocks whose three tables are in
    RLE_Mode are read to the end (their bit stream is the extra bits alone), which is where the repeat-offset codes are looked for."""
    pos = 0
    while pos < len(payload):
        if payload[pos + 1:pos + 4] == b"\x2a\x4d\x18":
            seen.add(("frame", "skippable"))
            pos += 8 + int.from_bytes(payload[pos + 4:pos + 8], "little")
            continue
        assert payload[pos:pos + 4] == MAGIC
        d = payload[pos + 4]
        single, fcs = (d >> 5) & 1, [1 if (d >> 5) & 1 else 0, 2, 4, 8][d >> 6]
        seen.add(("fcs", fcs, "single" if single else "window"))
        seen.add(("dict", [0, 1, 2, 4][d & 3]))
        pos += 5 + (0 if single else 1) + [0, 1, 2, 4][d & 3] + fcs
        last = 0
        while not last:
            h = int.from_bytes(payload[pos:pos + 3], "little")
            last, btype, size = h & 1, (h >> 1) & 3, h >> 3
            seen.add(("block", btype))
            pos += 3
            if btype == 2:
                walk_block(payload[pos:pos + size], seen)
            pos += 1 if btype == 1 else size
        if d & 4:
            seen.add(("frame", "checksum"))
            pos += 4
    assert pos == len(payload)


def walk_block(b, seen):
    ltype, fmt = b[0] & 3, (b[0] >> 2) & 3
    if ltype < 2:
        fmt = 0 if fmt in (0, 2) else fmt
        hdr = {0: 1, 1: 2, 3: 3}[fmt]
        regen = int.from_bytes(b[:hdr], "little") >> (3 if fmt == 0 else 4)
        q = hdr + (regen if ltype == 0 else 1)
    else:
        bits = {0: 10, 1: 10, 2: 14, 3: 18}[fmt]
        hdr = {10: 3, 14: 4, 18: 5}[bits]
        q = hdr + ((int.from_bytes(b[:hdr], "little") >> (4 + bits)) & ((1 << bits) - 1))
        if ltype == 2:
            seen.add(("weights", "direct" if b[hdr] >= 128 else "fse"))
    seen.add(("literals", ltype, fmt))
    if b[q] < 128:
        form, n, q = 1, b[q], q + 1
    elif b[q] < 255:
        form, n, q = 2, ((b[q] - 128) << 8) + b[q + 1], q + 2
    else:
        form, n, q = 3, b[q + 1] + (b[q + 2] << 8) + 0x7F00, q + 3
    seen.add(("nseq", form))
    if not n:
        return
    modes = b[q]
    for w, name in enumerate(("ll", "of", "ml")):
        seen.add(("mode", name, (modes >> (6 - 2 * w)) & 3))
    if modes == 0b01010100:
        lc, oc, mc = b[q + 1], b[q + 2], b[q + 3]
        stream = int.from_bytes(b[q + 4:], "little")
        at = stream.bit_length() - 1   # the final-bit marker
        for _ in range(n):
            at -= oc
            value = (1 << oc) + ((stream >> at) & ((1 << oc) - 1))
            at -= ML_BITS[mc]
            at -= LL_BITS[lc]
            ll = LL_BASE[lc] + ((stream >> at) & ((1 << LL_BITS[lc]) - 1))
            if value <= 3:
                seen.add(("repeat", value, "ll0" if ll == 0 else "ll"))
        assert at == 0


def test_the_forms_were_really_produced():
    """A writer that silently falls back to the common form fails here."""
    seen = set()
    for payload, _ in VALID.values():
        walk(payload, seen)
    want = {("literals", t, f) for t in (0, 1) for f in (0, 1, 3)} | {("literals", t, f) for t in (2, 3) for f in (0, 1, 2, 3)}
    want |= {("mode", w, m) for w in ("ll", "of", "ml") for m in range(4)}
    want |= {("nseq", f) for f in (1, 2, 3)}
    want |= {("repeat", c, l) for c in (1, 2, 3) for l in ("ll0", "ll")}
    want |= {("block", t) for t in (0, 1, 2)}
    want |= {("fcs", 4, "single"), ("fcs", 1, "single"), ("fcs", 2, "single"), ("fcs", 8, "single"), ("fcs", 4, "window"), ("fcs", 0, "window")}
    want |= {("dict", w) for w in (0, 1, 2, 4)} | {("frame", "skippable"), ("frame", "checksum"), ("weights", "direct"), ("weights", "fse")}
    assert not want - seen, sorted(want - seen, key=str)


def test_the_writer_against_a_real_encoder_where_the_spelling_is_forced():
    """Incompressible bytes at any level are one Raw_Block in a Single_Segment frame: the writer's bytes are libzstd's."""
    data = rnd(300, 200)
    assert Frame(fcs_bytes=1).raw(data, last=True).finish() == pa.Codec("zstd", compression_level=1).compress(data, asbytes=True)
