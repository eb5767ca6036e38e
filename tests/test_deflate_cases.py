"""Hand-built raw DEFLATE streams (tests/deflate_enc.py) and who accepts them.  The tables of this module are what
tests/test_gpu_deflate.py pushes through the DEFLATE kernels; here, without a GPU, every case is first shown to mean what
its name says: Python's zlib -- an independent inflate -- and the CPU oracle (oracle/oo_codecs.c) must both return the
writer's own model of the plain bytes for a VALID case, and both reject a MALFORMED one.

A chunk may expand to CAP bytes: what the oracle (and the library, on its second run) gives a DEFLATE chunk.  zlib knows
no such limit, so the two cases that overrun it are in ZLIB_DIFFERS, where only the oracle is asserted.

A third table, ORACLE_ACCEPTS, holds what fits neither rule: streams with a lone code whose length is not 1.  The oracle -- this
project's authority -- takes a lone code of any length, as puff does, and so must the kernels; zlib rejects it.  There the oracle
must return the model's bytes and zlib must refuse, each case with its reason.  HCLEN = 4 cannot be valid: only the symbols 16, 17, 18 and 0 then have codes, every
length is zero and there is no end-of-block code -- that header is a MALFORMED case here, HCLEN = 5 the smallest valid."""
import zlib

import numpy as np
import pytest

import oracle_lib as O
from deflate_enc import (DBASE, DEXT, LBASE, LEXT, Deflate, M, RawDist, RawLL, cut_bits, kraft, split_lengths)

CAP = 1 << 22

VALID = {}       # name -> (stream, plain)
MALFORMED = {}   # name -> stream
ORACLE_ACCEPTS = {}   # name -> (stream, plain, why zlib refuses what the oracle takes)
ZLIB_DIFFERS = {
    "over_capacity_by_a_literal": "zlib has no output limit: the 4 MiB a chunk may expand to is the ORC reader's",
    "over_capacity_by_a_match": "zlib has no output limit: the 4 MiB a chunk may expand to is the ORC reader's",
}


def valid(name, d, trailing=b""):
    assert name not in VALID
    VALID[name] = (d.finish(trailing), d.plain())


def malformed(name, stream):
    assert name not in MALFORMED
    MALFORMED[name] = d_bytes(stream)


def d_bytes(x):
    return x.finish() if isinstance(x, Deflate) else bytes(x)


def rnd(seed, n, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, n, dtype=np.uint8).tobytes()


# ---- lengths and distances --------------------------------------------------------------------------------------------
def every_length_symbol():
    toks = list(b"0123456789abcdef")
    for s in range(29):
        lo, hi = LBASE[s], LBASE[s] + (1 << LEXT[s]) - 1
        toks += [M(lo, 1 + s % 16, lsym=257 + s), 65 + s, M(hi, 16 - s % 16, lsym=257 + s)]
    return toks


def every_distance_symbol():
    toks = []
    for s in range(30):
        lo, hi = DBASE[s], DBASE[s] + (1 << DEXT[s]) - 1
        toks += [M(3 + s, lo), 97 + s % 26, M(40 - s, hi)]
    return toks


valid("length_symbols_fixed", Deflate().fixed(every_length_symbol(), final=True))
valid("length_symbols_dynamic", Deflate().auto_dynamic(every_length_symbol(), final=True))
# distance 32768 is symbol 29 at its highest extra bits; the source of every far match lies in a STORED block ...
valid("distance_symbols_fixed_from_stored", Deflate().stored(rnd(1, 32768)).fixed(every_distance_symbol(), final=True))
# ... and in an earlier Huffman block
valid("distance_symbols_dynamic_from_huffman", Deflate().auto_dynamic(list(rnd(2, 32768))).auto_dynamic(every_distance_symbol(), final=True))
valid("distance_32768_first_token_of_a_block", Deflate().fixed(list(rnd(3, 32768, 0, 144))).fixed([M(258, 32768), M(3, 32768)], final=True))
valid("length3_distance1", Deflate().fixed([0x5A, M(3, 1)], final=True))
valid("length258_distances_1_to_8", Deflate().fixed(
    list(b"abcdefgh") + [t for k in range(1, 9) for t in (M(258, k), M(258, k, lsym=284), 48 + k)], final=True))
valid("length258_both_spellings_dynamic", Deflate().auto_dynamic(list(b"xy") + [M(258, 1), M(258, 2, lsym=284)] * 6, final=True))
valid("distance_equals_bytes_so_far", Deflate().fixed(list(b"abcde") + [M(5, 5), M(10, 10), M(258, 20), M(3, 278)], final=True))
valid("distance_equals_bytes_so_far_across_blocks",
      Deflate().fixed(list(b"abcde")).stored(b"fgh").auto_dynamic([M(8, 8), M(16, 16)]).fixed([M(258, 32)], final=True))


# ---- code lengths 1 to 15 on both sides; the length and distance symbols among the long ones ---------------------------
def codes_1_to_15():
    ll = [0] * 286
    for k in range(10):
        ll[k] = k + 1          # literals 0..9: 1..10 bits (the fast table)
    for sym, l in ((256, 11), (257, 12), (270, 13), (285, 14), (281, 15), (284, 15)):
        ll[sym] = l
    dl = [0] * 30
    for sym, l in zip((0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 15, 20, 27, 28, 29), list(range(1, 16)) + [15]):
        dl[sym] = l
    assert kraft(ll) == 32768 and kraft(dl) == 32768
    toks = list(range(10)) * 4
    toks += [M(3, 1), M(23, 2), M(258, 3), M(131, 4), M(257, 5, lsym=284)]
    toks += [M(3, d) for d in (6, 8, 12, 16, 24, 30, 40)]
    toks += list(range(10)) * 400 + [M(24, 200), M(3, 1100), M(258, 1)]
    toks += list(range(10)) * 3000 + [M(162, 13000)]
    # 15 + 5 + 15 + 13 = 48 bits: length symbol 284 (15-bit code, 5 extra), distance symbols 28 and 29 (15-bit codes, 13 extra)
    toks += [M(257, 24576, lsym=284), 3, M(227, 24577, lsym=284), M(258, 32768, lsym=284), M(230, 16385, lsym=284), 7]
    return toks, ll, dl


_t, _ll, _dl = codes_1_to_15()
_d = Deflate().dynamic(_t, _ll, _dl, final=True)
valid("codes_of_1_to_15_bits", _d)


def many_long_codes():
    """All 286 + 30 symbols in use, four (three) of them short and the rest 11 to 15 bits: the long-code search by rank."""
    lens = split_lengths(286)
    short = [32, 101, 97, 116]
    ll = [0] * 286
    order = short + [s for s in range(286) if s not in short]
    for s, l in zip(order, lens):
        ll[s] = l
    dlens = split_lengths(30)
    dl = [0] * 30
    for s, l in zip([0, 3, 6] + [s for s in range(30) if s not in (0, 3, 6)], dlens):
        dl[s] = l
    assert kraft(ll) == 32768 and kraft(dl) == 32768 and sum(1 for l in ll if l > 10) > 200 and sum(1 for l in dl if l > 10) >= 8
    rng = np.random.default_rng(15)
    toks = list(range(256)) * 2 + list(rnd(16, 33000))
    for s in range(29):
        for ds in range(30):
            toks.append(M(LBASE[s] + int(rng.integers(0, 1 << LEXT[s])), DBASE[ds] + int(rng.integers(0, 1 << DEXT[ds])), lsym=257 + s))
            if (s + ds) % 3 == 0:
                toks.append(int(rng.integers(0, 256)))
    return toks, ll, dl


_t, _ll, _dl = many_long_codes()
valid("long_codes_for_every_symbol", Deflate().dynamic(_t, _ll, _dl, final=True))


# ---- streams whose codes do not self-synchronise -------------------------------------------------------------------------
def nonsync_literals():
    """63 literals of 6 bits, an unused literal and the end of block of 7: the Kraft sum is 1, every token 6 bits long, and a decoder
    that starts between two tokens stays there (it finds its way back only through the one 6-bit prefix of the 7-bit codes)."""
    ll = [6] * 63 + [7] + [0] * 192 + [7]
    assert kraft(ll) == 32768
    return Deflate().dynamic(list(rnd(21, 56000, 0, 63)), ll, [0], final=True)


def nonsync_phase_locked(threads, windows):
    """The same with sparse matches, placed so that NO guess of the token stage is ever right: with `threads` segments of
    256 bits to a window, every window's first segment holds one match of 9 bits (an odd number), and every literal's code
    starts with a 0 bit.  All tokens behind the match start an odd number of bits behind the window's first bit, every guess
    (a multiple of 256) an even number: a guess lies 1, 3 or 5 bits inside a literal.  The 7-bit codes start with 111110 or
    111111.  A decoder 2 to 5 bits inside a literal has that literal's successor's first bit, a 0, among the first five of its
    six bits: it reads a 6-bit literal and stays where it is.  One bit inside a literal the 0 is the sixth bit: at most it reads
    111110 and one bit more (literal 62, or an end of block that stops it), which puts it 2 bits inside a literal, for good.
    It is never 0 bits inside: no decoder falls in step by itself.  Segment k is right only once segment k - 1 is, and its
    end then moves: threads - 1 rounds."""
    ll = [6] * 62 + [7] + [0] * 193 + [7, 7, 7]   # 7 bits: literal 62 (unused), end of block, lengths 3 and 4
    dl = [1, 0, 0, 0, 1]                            # distance 1, and distances 5..6 with their one extra bit
    assert kraft(ll) == 32768 and kraft(dl) == 32768
    lits = iter(rnd(22 + threads, 400000, 0, 32))
    toks, pos = [], 0
    for _ in range(windows):
        edge = pos + threads * 256
        toks += [next(lits) for _ in range(6)] + [M(3, 5)]
        pos += 6 * 6 + 9
        while pos < edge:   # the window's last segment decodes while tokens START before the edge
            toks.append(next(lits))
            pos += 6
    toks += [next(lits) for _ in range(100)]
    return Deflate().dynamic(toks, ll, dl, final=True)


valid("nonsync_6bit_literals", nonsync_literals())
valid("nonsync_sparse_matches_64_segments", nonsync_phase_locked(64, 22))
valid("nonsync_sparse_matches_256_segments", nonsync_phase_locked(256, 6))
for _n in ("nonsync_6bit_literals", "nonsync_sparse_matches_64_segments", "nonsync_sparse_matches_256_segments"):
    assert len(VALID[_n][0]) >= 40 * 1024


# ---- blocks and window edges ---------------------------------------------------------------------------------------------
def fixed_literals_to(d, end_bit, seed, tail=(), tail_bits=0):
    """A fixed block (not the last) of literals, then the tokens of `tail` (tail_bits bits), whose end-of-block code ENDS at bit
    `end_bit` of the stream."""
    room = end_bit - d.bitpos - 3 - 7 - tail_bits
    y = next(y for y in range(8) if (room - 9 * y) % 8 == 0 and room - 9 * y >= 0)   # 9-bit literals: 144..255
    x = (room - 9 * y) // 8                                                              # 8-bit literals: 0..143
    toks = list(rnd(seed, x, 0, 144))
    for k in range(y):
        toks.insert((k * 37) % (len(toks) + 1), 200 + k)
    d.fixed(toks + list(tail))
    assert d.bitpos == end_bit
    return d


# the first window of a chunk's first Huffman block starts behind the 3 header bits: it ends at bit 3 + 256 * threads
for _threads in (64, 256):
    # (the code is 7 bits long: at +7 it STARTS on the edge, the next window's first token and the block's last; at +8 one bit behind it)
    for _off in (-1, 0, 1, 3, 7, 8):
        _d = fixed_literals_to(Deflate(), 3 + 256 * _threads + _off, 30 + _off)
        _d.fixed([M(100, 7), 1, 2, 3, M(258, 3 + 256 * _threads // 16)], final=True)
        valid("end_of_block_%+d_bits_from_the_%d_byte_window_edge" % (_off, 32 * _threads), _d)
    # the window's last token is a match that starts one bit before the edge and reaches 21 / 23 bits into the slack, the end-of-block
    # code behind it: 8 bits for length 258, 5 + 9 / 5 + 11 for the distance
    _far = 2000 if _threads == 64 else 8000
    _d = fixed_literals_to(Deflate(), 3 + 256 * _threads - 1 + 8 + 5 + (9 if _threads == 64 else 11) + 7, 35, tail=[M(258, _far)],
                           tail_bits=8 + 5 + (9 if _threads == 64 else 11))
    _d.fixed([M(3, 1), 4], final=True)
    valid("match_across_the_%d_byte_window_edge_then_end_of_block" % (32 * _threads), _d)
    # a dynamic header across the byte the window would have ended at
    _d = fixed_literals_to(Deflate(), 256 * _threads - 150, 40)
    _d.auto_dynamic(list(rnd(41, 3000)) + [M(9, 2999), M(258, 1)], final=True)
    assert _d.header_end > 256 * _threads + 100
    valid("dynamic_header_across_byte_%d" % (32 * _threads), _d)

# the final end-of-block code ends on the last bit of the input: 3 + 6 * 9 + 7 = 64 bits
_last_bit = lambda: Deflate().fixed([200, 201, 202, 203, 204, 205], final=True)
assert _last_bit().bitpos == 64
valid("ends_on_the_last_bit_of_the_input", _last_bit())
valid("ends_on_the_last_bit_then_zero_bytes", _last_bit(), trailing=bytes(5))
valid("ends_on_the_last_bit_then_garbage", _last_bit(), trailing=b"\xff\x07garbage\xfe")
valid("ends_in_mid_byte_then_garbage", Deflate().fixed(list(b"tail"), final=True), trailing=b"\x05\x00\xff")
valid("long_stream_ends_on_the_last_bit", fixed_literals_to(Deflate(), 8 * 5000 - 64, 45).fixed([200, 201, 202, 203, 204, 205], final=True))

# ---- stored blocks -------------------------------------------------------------------------------------------------------
valid("stored_empty_in_front_between_behind",
      Deflate().stored().fixed(list(b"sync flush")).stored().stored().auto_dynamic(list(b"between") + [M(10, 7)]).stored(final=True))
valid("stored_65535", Deflate().fixed(list(b"ab")).stored(rnd(50, 65535)).fixed([M(258, 32768), M(4, 1)], final=True))
valid("stored_then_match_first", Deflate().fixed(list(b"0123456789")).stored(b"ABCDEFGHIJKLMNOP").fixed([M(20, 26), 33, M(3, 1)], final=True))
valid("match_then_stored_then_match_first", Deflate().fixed(list(b"01234") + [M(7, 5)]).stored(b"xyz").auto_dynamic([M(9, 15), M(3, 3)], final=True))
valid("stored_first_then_match_first", Deflate().stored(b"abcdefgh").fixed([M(8, 8)], final=True))
valid("stored_then_stored_then_match", Deflate().stored(b"abc").stored(rnd(51, 3000)).stored(b"").fixed([M(258, 3003), 9], final=True))
valid("stored_blocks_only", Deflate().stored(rnd(52, 1000)).stored(b"").stored(rnd(53, 17)).stored(rnd(54, 4096), final=True))
valid("stored_at_every_bit_offset",
      Deflate().fixed([1]).stored(b"a").fixed([2, 200]).stored(b"b").fixed([200, 201]).stored(b"c").fixed([M(3, 2)]).stored(b"d", final=True))
valid("empty_fixed_block", Deflate().fixed([], final=True))
assert VALID["empty_fixed_block"][0] == b"\x03\x00"
valid("empty_final_stored_block", Deflate().stored(final=True))
valid("empty_blocks_of_every_type", Deflate().fixed([]).stored().dynamic([], [0] * 256 + [1], [0]).fixed([], final=True))

# ---- headers -------------------------------------------------------------------------------------------------------------
valid("hlit_257_hdist_1_no_distance_code", Deflate().dynamic(list(b"abracadabra" * 30), [0] * 97 + [2, 2, 3, 3] + [0] * 13 + [3] + [0] * 141 + [3], [0], final=True))
valid("one_distance_code_of_1_bit", Deflate().dynamic(list(b"ab") + [M(3, 1), 98, M(4, 1), M(3, 1), M(4, 1)], [0] * 97 + [2, 2] + [0] * 157 + [2, 3, 3] + [0] * 26 + [0], [1], final=True))
valid("one_distance_code_of_1_bit_symbol_4", Deflate().dynamic(list(b"abcdef") + [M(258, 5), M(258, 6), 97, M(258, 5)], [0] * 97 + [3] * 6 + [0] * 153 + [3] + [0] * 28 + [3], [0, 0, 0, 0, 1], final=True))
valid("only_an_end_of_block_code", Deflate().stored(b"12345678").dynamic([], [0] * 256 + [1], [0], final=True))
# a repeat of the previous length (16) that starts in the literal/length list and ends in the distance list ...
valid("repeat_16_across_the_two_lists", Deflate().dynamic(
    [97] * 40 + [M(3, 4), M(4, 1), M(3, 3)], [0] * 97 + [1] + [0] * 158 + [2, 3, 3], [3, 3, 3, 3, 1], final=True,
    cl_syms=[(18, 97 - 11), (1, 0), (18, 127), (18, 20 - 11), (2, 0), (3, 0), (16, 2), (1, 0)]))
# ... and a run of zeros (18)
valid("repeat_18_across_the_two_lists", Deflate().dynamic(
    [97] * 60 + [M(3, 33), M(3, 49)], [0] * 97 + [1] + [0] * 158 + [2, 2] + [0] * 13, [0] * 10 + [1, 1], final=True,
    cl_syms=[(18, 97 - 11), (1, 0), (18, 127), (18, 20 - 11), (2, 0), (2, 0), (18, 23 - 11), (1, 0), (1, 0)]))
# HCLEN 5 (the least that can be valid: 16, 17, 18, 0, 8): 256 codes of 8 bits
valid("hclen_5", Deflate().dynamic(list(rnd(60, 500, 0, 255)), [8] * 255 + [0, 8], [0], final=True,
                                   cl_lens=[1] + [0] * 7 + [2] + [0] * 9 + [2], hclen=5, cl_syms=[(8, 0)] * 255 + [(0, 0), (8, 0), (0, 0)]))
valid("hclen_19", Deflate().dynamic(list(range(10)) * 3 + [M(3, 1)], codes_1_to_15()[1], codes_1_to_15()[2], final=True, hclen=19))


# ---- a lone code that is not 1 bit long: the oracle (as puff) takes it, zlib does not ------------------------------------------------
def oracle_accepts(name, d, why):
    assert name not in ORACLE_ACCEPTS and name not in VALID and name not in MALFORMED
    ORACLE_ACCEPTS[name] = (d.finish(), d.plain(), why)


_ll3 = [0] * 97 + [1] + [0] * 158 + [2, 3, 3]   # 'a', end of block, lengths 3 and 4
oracle_accepts("lone_distance_code_of_2_bits", Deflate().dynamic([97, 97, M(3, 1), 97, M(4, 1), M(3, 1)], _ll3, [2], final=True),
               "zlib takes an incomplete distance code only when its one code is 1 bit long")
oracle_accepts("lone_distance_code_of_5_bits_symbol_9", Deflate().dynamic([97] * 30 + [M(4, 25), 97, M(3, 32), M(4, 29)], _ll3, [0] * 9 + [5], final=True),
               "zlib takes an incomplete distance code only when its one code is 1 bit long")
oracle_accepts("lone_distance_code_of_15_bits", Deflate().dynamic([97] * 3 + [M(4, 2), 97, M(3, 2)] * 5, _ll3, [0, 15], final=True),
               "zlib takes an incomplete distance code only when its one code is 1 bit long")
oracle_accepts("lone_end_of_block_code_of_2_bits", Deflate().stored(b"12345678").dynamic([], [0] * 256 + [2], [0], final=True),
               "zlib takes an incomplete literal/length code only when its one code is 1 bit long")
oracle_accepts("lone_end_of_block_code_of_12_bits", Deflate().fixed(list(b"abcdefgh")).dynamic([], [0] * 256 + [12], [0]).fixed([M(8, 8)], final=True),
               "zlib takes an incomplete literal/length code only when its one code is 1 bit long")


# ---- a seeded soup of blocks of all three types ------------------------------------------------------------------------------
def soup_tokens(rng, have, budget):
    alphabet = rng.permutation(256)[:int(rng.choice([2, 17, 64, 256]))]
    weights = 1.0 / (1 + np.arange(len(alphabet))) ** float(rng.choice([0.0, 1.0, 2.5]))
    weights /= weights.sum()
    toks, made = [], 0
    while made < budget:
        if have + made == 0 or rng.random() < 0.6:
            n = int(rng.choice([1, 1, 2, 5, 40]))
            toks += [int(x) for x in rng.choice(alphabet, n, p=weights)]
            made += n
            continue
        length = int(rng.choice([3, 4, 5, 10, 11, 18, 66, 130, 227, 257, 258])) if rng.random() < 0.7 else int(rng.integers(3, 259))
        far = min(have + made, 32768)
        pick = rng.random()
        dist = int(rng.integers(1, min(far, 8) + 1)) if pick < 0.35 else int(rng.integers(1, min(far, 300) + 1)) if pick < 0.7 else int(rng.integers(1, far + 1))
        toks.append(M(length, dist, lsym=284 if length == 258 and rng.random() < 0.5 else None))
        made += length
    return toks, made


def soup(seed, total=250000):
    rng = np.random.default_rng(seed)
    d = Deflate()
    while len(d.out) < total:
        left = total - len(d.out)
        kind = int(rng.integers(0, 4))
        if kind == 0:
            d.stored(rng.integers(0, 256, min(left, int(rng.choice([0, 1, 7, 300, 5000, 65535]))), dtype=np.uint8).tobytes())
            continue
        toks, _ = soup_tokens(rng, len(d.out), min(left, int(rng.choice([0, 10, 500, 6000, 40000]))))
        if kind == 1:
            d.fixed(toks)
        else:
            d.auto_dynamic(toks)
    [lambda: d.stored(final=True), lambda: d.fixed([], final=True), lambda: d.auto_dynamic([], final=True)][int(rng.integers(0, 3))]()
    return d


for _seed in (1, 2, 3):
    valid("soup_seed_%d" % _seed, soup(_seed))

assert all(len(p) <= 262144 for _, p in VALID.values())

# ---- malformed ---------------------------------------------------------------------------------------------------------------
malformed("block_type_3", Deflate().reserved(final=True).finish() + bytes(8))
malformed("block_type_3_behind_a_block", Deflate().fixed(list(b"fine")).reserved(final=True).finish() + bytes(8))
malformed("stored_wrong_nlen", Deflate().fixed(list(b"ok")).stored(b"payload", final=True, nlen=0x1234))
malformed("stored_nlen_equal_to_len", Deflate().stored(b"payload", final=True, nlen=7))
malformed("stored_length_past_the_input", Deflate().stored(rnd(70, 300), final=True).finish()[:-1])
malformed("stored_header_cut", Deflate().fixed(list(b"ok")).stored(b"payload", final=True).finish()[:5])
malformed("fixed_symbol_286", Deflate(check=False).fixed(list(b"abc") + [RawLL(286)] + list(b"def"), final=True))
malformed("fixed_symbol_287", Deflate(check=False).fixed(list(b"abc") + [RawLL(287)] + list(b"def"), final=True))
malformed("fixed_distance_30", Deflate(check=False).fixed(list(b"abc") + [RawDist(3, 30)] + list(b"def"), final=True))
malformed("fixed_distance_31", Deflate(check=False).fixed(list(b"abc") + [RawDist(3, 31)] + list(b"def"), final=True))
malformed("distance_one_too_far_first_block", Deflate(check=False).fixed(list(b"abcde") + [M(3, 6)], final=True))
malformed("distance_one_too_far_behind_a_block_edge", Deflate(check=False).fixed(list(b"abcde")).fixed([M(3, 6)], final=True))
malformed("distance_one_too_far_behind_a_stored_block", Deflate(check=False).stored(b"abcde").auto_dynamic([1, 2, M(258, 8)], final=True))
malformed("distance_in_an_empty_output", Deflate(check=False).fixed([M(3, 1)], final=True))
_full = [0] + [M(258, 1)] * 16256 + [M(255, 1)]   # 1 + 16256 * 258 + 255 = 4 MiB
malformed("over_capacity_by_a_literal", Deflate().fixed(_full + [1], final=True))
malformed("over_capacity_by_a_match", Deflate().fixed(_full + [M(3, 1)], final=True))
assert len(Deflate().fixed(_full, final=True).plain()) == CAP
# headers
_ab = [0] * 97 + [2, 2]   # 'a', 'b'
malformed("no_code_for_end_of_block", Deflate(check=False).dynamic([97, 98], _ab + [2, 2] + [0] * 156, [0], final=True, eob=False))
malformed("literal_length_code_oversubscribed", Deflate(check=False).dynamic([97], [0] * 97 + [1, 1] + [0] * 157 + [1], [0], final=True))
malformed("distance_code_oversubscribed", Deflate(check=False).dynamic([97], _ab + [0] * 157 + [1], [1, 1, 1], final=True, eob=False))
malformed("code_length_code_oversubscribed", Deflate(check=False).dynamic([97], _ab + [0] * 157 + [1], [0], final=True, eob=False,
                                                                         cl_lens=[1, 1, 1] + [0] * 14 + [2, 2]))
malformed("code_length_code_incomplete", Deflate(check=False).dynamic([97], [0] * 97 + [2, 2] + [0] * 157 + [1], [0], final=True,
                                                                      cl_lens=[2, 2, 2] + [0] * 15 + [3]))
malformed("literal_length_code_incomplete_two_symbols", Deflate().dynamic([97], [0] * 97 + [2] + [0] * 158 + [2], [0], final=True))
malformed("literal_length_code_incomplete_unused_symbol", Deflate().dynamic([97], [0] * 97 + [1] + [0] * 158 + [2, 3], [0], final=True))
malformed("distance_code_incomplete_two_symbols", Deflate().dynamic([97, M(3, 1)], [0] * 97 + [1] + [0] * 158 + [2, 2], [2, 2], final=True))
malformed("hlit_287", Deflate().dynamic([97], [0] * 97 + [1] + [0] * 158 + [2, 2] + [0] * 28, [0], final=True, hlit=287))
malformed("hlit_288", Deflate().dynamic([97], [0] * 97 + [1] + [0] * 158 + [2, 2] + [0] * 29, [0], final=True, hlit=288))
malformed("hdist_31", Deflate().dynamic([97], [0] * 97 + [1] + [0] * 158 + [2, 2], [1] + [0] * 30, final=True, hdist=31))
malformed("hdist_32", Deflate().dynamic([97], [0] * 97 + [1] + [0] * 158 + [2, 2], [1] + [0] * 31, final=True, hdist=32))
malformed("repeat_16_first", Deflate(check=False).dynamic([], [0] * 256 + [1], [0], final=True, eob=False,
                                                         cl_syms=[(16, 0), (18, 127), (18, 116 - 11), (1, 0), (0, 0)], cl_lens=[1] + [2] + [0] * 14 + [3, 0, 3]))
malformed("repeat_18_overruns_the_lists", Deflate(check=False).dynamic([], [0] * 256 + [1], [0], final=True, eob=False,
                                                                       cl_syms=[(18, 127), (18, 118 - 11), (1, 0), (18, 0)]))
malformed("repeat_16_overruns_the_lists", Deflate(check=False).dynamic([], [0] * 254 + [2, 2, 1], [0], final=True, eob=False,
                                                                       cl_syms=[(18, 127), (18, 116 - 11), (2, 0), (2, 0), (1, 0), (16, 3)]))
malformed("hclen_4_has_no_lengths_but_zero", Deflate(check=False).dynamic([], [0] * 257, [0], final=True, eob=False,
                                                                          cl_lens=[1] + [0] * 17 + [1], hclen=4))
malformed("length_symbol_without_a_distance_code", Deflate(check=False).dynamic([97, RawLL(257), 97], [0] * 97 + [1] + [0] * 158 + [2, 2], [0], final=True))
# the input ends inside a block: 3 + 5 * 9 = 48 bits, no end-of-block code (7 zero bits of padding would be one)
malformed("no_end_of_block_code", Deflate().fixed([200, 201, 202, 203, 204], final=True, eob=False))
malformed("no_end_of_block_code_long", fixed_literals_to(Deflate(), 8 * 3000, 71).fixed([200, 201, 202, 203, 204], final=True, eob=False))
malformed("no_final_block", Deflate().fixed(list(b"there is no last block")))
malformed("no_final_block_on_the_last_bit", Deflate().fixed([200, 201, 202, 203, 204, 205]))
malformed("no_final_block_behind_a_stored_block", Deflate().fixed(list(b"abc")).stored(b"defgh"))
malformed("match_cut_in_its_distance_bits", cut_bits(Deflate().fixed(list(rnd(72, 40, 0, 144)) + [M(3, 30)], final=True).finish(), 3 + 320 + 7 + 5 + 2))


# truncation sweep: one dynamic block of about 300 bytes, cut in every byte of its header and at evenly spread places behind it
def sweep_stream():
    rng = np.random.default_rng(80)
    words = [b"AIR", b"FOB", b"MAIL", b"RAIL", b"REG AIR", b"SHIP", b"TRUCK", b"NONE", b"TAKE BACK RETURN"]
    toks = []
    for _ in range(44):
        toks += list(words[int(rng.integers(0, len(words)))] + b" ")
    toks += [M(12, 40), M(3, 1), M(100, 200)] + list(rnd(81, 80)) + [M(258, 64, lsym=284)]
    return Deflate().auto_dynamic(toks, final=True)


_sw = sweep_stream()
SWEEP = _sw.finish()
SWEEP_PLAIN = _sw.plain()
SWEEP_HEADER_BYTES = (_sw.header_end + 7) // 8
assert 250 <= len(SWEEP) <= 400, len(SWEEP)
_cuts = set(range(0, SWEEP_HEADER_BYTES + 1)) | {SWEEP_HEADER_BYTES + (k * (len(SWEEP) - 1 - SWEEP_HEADER_BYTES)) // 47 for k in range(48)}
for _c in sorted(_cuts):
    assert _c < len(SWEEP)
    malformed("cut_at_byte_%03d" % _c, SWEEP[:_c])
valid("the_stream_of_the_truncation_sweep", _sw)


# ---- the judges ------------------------------------------------------------------------------------------------------------------
def zlib_inflate(stream):
    """(plain, None) when Python's zlib takes the stream as one complete raw DEFLATE stream, else (None, why)."""
    z = zlib.decompressobj(-15)
    try:
        out = z.decompress(stream)
    except zlib.error as e:
        return None, str(e)
    return (out, None) if z.eof else (None, "the stream does not end")


@pytest.mark.parametrize("name", list(ORACLE_ACCEPTS))
def test_oracle_accepts_what_zlib_refuses(name):
    stream, plain, why = ORACLE_ACCEPTS[name]
    assert why and zlib_inflate(stream)[0] is None, (name, "zlib takes it after all: it belongs in VALID")
    assert O.codec("zlib", stream, CAP) == plain, (name, "the oracle does not return the model's bytes")
    assert O.codec("zlib", stream, len(plain) - 1) is None, (name, "a slot one byte short")


def test_the_tables_are_what_the_issue_asks_for():
    assert len(VALID) >= 50 and len(MALFORMED) >= 48 + 30
    assert not set(ZLIB_DIFFERS) & set(VALID)
    assert set(ZLIB_DIFFERS) <= set(MALFORMED)
    assert 10 * len(ZLIB_DIFFERS) <= len(MALFORMED)
    assert sum(1 for n in MALFORMED if n.startswith("cut_at_byte_")) >= 48


@pytest.mark.parametrize("name", list(VALID))
def test_valid_case_is_accepted_by_zlib_and_the_oracle(name):
    stream, plain = VALID[name]
    got, why = zlib_inflate(stream)
    assert got is not None, (name, why)
    assert got == plain, (name, "zlib differs from the model", len(got), len(plain))
    o = O.codec("zlib", stream, CAP)
    assert o is not None, (name, "the oracle rejects it")
    assert o == plain, (name, "the oracle differs from the model", len(o), len(plain))
    if len(plain):
        assert O.codec("zlib", stream, len(plain)) == plain, (name, "a slot of exactly the plain size")
        assert O.codec("zlib", stream, len(plain) - 1) is None, (name, "a slot one byte short")


@pytest.mark.parametrize("name", list(MALFORMED))
def test_malformed_case_is_rejected_by_zlib_and_the_oracle(name):
    stream = MALFORMED[name]
    if name not in ZLIB_DIFFERS:
        got, why = zlib_inflate(stream)
        assert got is None, (name, "zlib accepts it", len(got))
    else:
        assert zlib_inflate(stream)[0] is not None, (name, "zlib agrees after all: take it out of ZLIB_DIFFERS")
    assert O.codec("zlib", stream, CAP) is None, (name, "the oracle accepts it")


def test_garbage_behind_the_last_block_is_left_alone_by_zlib_too():
    for name in ("ends_on_the_last_bit_then_zero_bytes", "ends_on_the_last_bit_then_garbage", "ends_in_mid_byte_then_garbage"):
        z = zlib.decompressobj(-15)
        assert z.decompress(VALID[name][0]) == VALID[name][1] and z.eof and len(z.unused_data) >= 3, name


def test_the_writer_reproduces_zlib_stored_output():
    """The writer against a real encoder where the spelling is forced: level 0 is one stored block."""
    data = b"abcabcabcabc hello hello hello " * 3
    c = zlib.compressobj(0, zlib.DEFLATED, -15)
    assert Deflate().stored(data, final=True).finish() == c.compress(data) + c.flush()
