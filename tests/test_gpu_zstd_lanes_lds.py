"""GPU parity of zstd_seq_quads_kernel (device/zstd_lanes.h) at the shapes where its LDS layout can go wrong: the tables of the
sixteen chains of a wavefront, their bit-stream rings, and the way the decoded values change lanes on their way out (put_vals).

Every block is written by tests/zstd_enc.py, which says what it must decode to; every chain of a call is a column of its own
(a DOUBLE column carries arbitrary bytes, see test_gpu_codecs.py), all columns of a call decode to the same number of bytes
(frames are filled up with RLE blocks of zeros), and every column is compared byte for byte with the writer's model and batch
by batch with the oracle.  ORCGPU_ZSTD_LANES=1 forces the table-scale kernels, which the library takes by itself only for calls
with tens of millions of sequences.

  * chains per call 1, 15, 16, 17, 33: a partly filled last wavefront, exactly one, idle quads that follow chain 0;
  * sequences per block 1, 15, 16, 17, 32, 33 (a partial last group of put_vals, the even padding of the record array) and 2100
    at the largest accuracy logs (LL 9, ML 9, OF 8: the chain's tables use all their 1280 cells);
  * bit streams shorter than one 64-byte block, and of exactly one ring, one ring + 1 and three rings -- for both ring sizes the
    kernel can be built with (256 and 512 bytes), so the list holds whichever the constant is;
  * a step of 74 bits (the `total > 57` branch) in a wavefront whose other chains take ordinary steps;
  * sixteen chains of different (LL, OF, ML) table modes and accuracy logs, predefined and RLE tables among them, in one wavefront;
  * a malformed bit stream among fifteen valid ones: no end mark, too short for the initial states, running dry, bits left over
    (the kernel's status words 21 to 24): the oracle's status for that column, every other column intact."""
import numpy as np
import pytest

import gpu_util as G
from test_gpu_codecs import DATA, DOUBLE
from test_gpu_deflate import block_size_for, chunk, values
from zstd_enc import BLOCK_MAX, PREDEF, Frame, Fse, RawLit, Rle, S

pytestmark = pytest.mark.gpu

PREFIX = 600           # random bytes in front of a compressed block: what its matches copy from
P, R = "predefined", "rle"
COUNTS = [1, 15, 16, 17, 32, 33]
# (LL, OF, ML): predefined, RLE, or the accuracy log of an FSE table
MODES = [(P, P, P), (R, R, R), (5, 5, 5), (6, 5, 6), (7, 6, 7), (8, 7, 8), (9, 8, 9), (P, 8, R), (R, P, 9), (9, R, P), (6, P, P), (P, 6, P), (P, P, 6),
         (R, 5, 9), (9, 5, R), (5, 8, 5)]
assert len(MODES) == 16 and len(set(MODES)) == 16


@pytest.fixture(autouse=True)
def lanes(monkeypatch):
    monkeypatch.setenv("ORCGPU_ZSTD_LANES", "1")


def spec(kind):
    return PREDEF if kind == P else Rle() if kind == R else Fse(log=kind)


def sequences(seed, n, modes=(P, P, P)):
    """n sequences behind PREFIX bytes and the literals they take.  An RLE table has one code: one literal length, offsets of one
    code (8 extra bits), one match length.  Otherwise mostly short lengths, now and then one with extra bits."""
    rng = np.random.default_rng(seed)
    ll_kind, of_kind, ml_kind = modes
    short, long_ = (21, 67) if ml_kind == 5 else (35, 131)   # (a table of 32 cells: at most 26 match-length codes)
    seqs = []
    for _ in range(n):
        ll = 2 if ll_kind == R else int(rng.integers(0, 16)) if rng.random() < 0.8 else int(rng.integers(16, 64))
        ml = 5 if ml_kind == R else int(rng.integers(3, short)) if rng.random() < 0.8 else int(rng.integers(35, long_))
        off = int(rng.integers(253, 509)) if of_kind == R else int(rng.integers(1, PREFIX + 1))
        seqs.append(S(ll, ml, off))
    return seqs


def open_frame(seed, seqs, modes=(P, P, P), tamper=None, check=True):
    """A frame of PREFIX raw bytes and one compressed block of `seqs` (raw literals); not closed yet (fill_up)."""
    rng = np.random.default_rng(seed + 1_000_000)
    f = Frame(fcs_bytes=4, single_segment=False, check=check)
    f.raw(rng.integers(0, 256, PREFIX, dtype=np.uint8).tobytes())
    lits = rng.integers(0, 256, sum(q.ll for q in seqs) + 3, dtype=np.uint8).tobytes()
    ll, of, ml = (spec(k) for k in modes)
    f.compressed(RawLit(lits), seqs, ll=ll, of=of, ml=ml, tamper=tamper)
    return f


def fill_up(frames):
    """Closes the frames with RLE blocks of zeros so that all decode to the same number of bytes, a multiple of eight."""
    total = (max(len(f.out) for f in frames) + 8) & ~7
    for f in frames:
        while total - len(f.out) > BLOCK_MAX:
            f.rle(0, BLOCK_MAX)
        f.rle(0, total - len(f.out), last=True)
    return total


def decode_call(frames, bad=()):
    """Every frame a column of one call.  The columns not in `bad` must decode to the model's bytes and the oracle's batches; the
    call's status is returned with the result."""
    total = fill_up(frames)
    bs = block_size_for(total)
    cols = [{"column_id": k + 1, "orc_type": DOUBLE, "encoding": 0} for k in range(len(frames))]
    streams = [(k + 1, DATA, chunk(f.finish())) for k, f in enumerate(frames)]
    res = G.gpu_decode(total // 8, cols, streams, compression="zstd", block_size=bs)
    try:
        if not bad:
            assert res.status()[0] == 0, res.status()
        for ci, f in enumerate(frames):
            if ci not in bad:
                assert values(res, ci) == f.plain(), ("column", ci, "not the model's bytes")
            G.assert_column_parity(res, ci, cols[ci], streams, total // 8, 8192, compression="zstd", block_size=bs, what=("column", ci))
        return res.status(), cols, streams, total, bs
    finally:
        res.free()


@pytest.mark.parametrize("n_chains", [1, 15, 16, 17, 33])
def test_chains_per_call(n_chains):
    """Chains of 1 .. 33 sequences and of every table mode share the wavefronts."""
    decode_call([open_frame(100 + k, sequences(100 + k, COUNTS[k % len(COUNTS)], MODES[k % 16]), MODES[k % 16]) for k in range(n_chains)])


@pytest.mark.parametrize("n_seq", COUNTS + [2100])
def test_sequences_per_block(n_seq):
    """One chain alone in its wavefront (the other fifteen quads follow it and store nothing); 2100 sequences at the largest logs."""
    modes = (9, 8, 9) if n_seq > 33 else (P, P, P)
    decode_call([open_frame(200 + n_seq, sequences(200 + n_seq, n_seq, modes), modes)])


def test_the_large_block_beside_short_ones():
    """All 1280 cells of one chain's tables in use while its fifteen neighbours' chains end early and decode on."""
    big = (9, 8, 9)
    decode_call([open_frame(300, sequences(300, 2100, big), big)] + [open_frame(301 + k, sequences(301 + k, COUNTS[k % len(COUNTS)], MODES[k]), MODES[k]) for k in range(15)])


_by_length = {}


def frame_with_bit_stream_of(n_bytes):
    """A block whose bit stream is exactly n_bytes long: offsets of one code (RLE table, 8 bits each), predefined length tables
    (their state bits vary), the count of sequences searched for.  A sequence adds 2 to 3 bytes, so most seeds pass over a given
    length: the first seed that meets it is taken."""
    if n_bytes in _by_length:
        return _by_length[n_bytes]
    modes = (P, R, P)
    for seed in range(400, 500):
        seqs = sequences(seed, n_bytes // 2 + 2, modes)
        got = {}

        def length(n):
            open_frame(seed, seqs[:n], modes, tamper=lambda name, b: got.__setitem__(name, len(b)) or b)
            return got["bits"]
        lo, hi = 1, len(seqs)
        while lo < hi:   # the first count whose stream is not shorter (lengths grow with the count, near enough)
            mid = (lo + hi) // 2
            if length(mid) < n_bytes:
                lo = mid + 1
            else:
                hi = mid
        for n in range(max(1, lo - 2), min(len(seqs), lo + 2) + 1):
            if length(n) == n_bytes:
                _by_length[n_bytes] = (seed, seqs[:n], modes)
                return _by_length[n_bytes]
    raise AssertionError("no block with a bit stream of %d bytes" % n_bytes)


@pytest.mark.parametrize("n_bytes", [40, 256, 257, 512, 513, 768, 1536])
def test_bit_stream_lengths(n_bytes):
    """Wrap-around of the ring and the copy of its first bytes behind its end: the stream alone, and beside fifteen others."""
    seed, seqs, modes = frame_with_bit_stream_of(n_bytes)
    decode_call([open_frame(seed, seqs, modes)])
    decode_call([open_frame(500 + k, sequences(500 + k, COUNTS[k % len(COUNTS)], MODES[k]), MODES[k]) for k in range(15)] + [open_frame(seed, seqs, modes)])


def test_a_step_of_74_bits_among_ordinary_ones():
    """test_zstd_cases.py's widest step (18 + 15 + 15 extra bits, 9 + 9 + 8 state bits), here with fifteen other chains in its wavefront:
    all of them go through the window-per-field branch in that step."""
    rng = np.random.default_rng(600)
    wide = Frame(fcs_bytes=4, single_segment=False)
    wide.raw(rng.integers(0, 256, BLOCK_MAX, dtype=np.uint8).tobytes()).raw(rng.integers(0, 256, 68000, dtype=np.uint8).tobytes())
    seqs = [S(1, 3, 1)] * 20 + [S(65535, 40000, (1 << 18) + 2000 - 3), S(1, 3, 1)] + [S(2, 4, 2)] * 5
    wide.compressed(RawLit(rng.integers(0, 256, 65600, dtype=np.uint8).tobytes()), seqs, ll=Fse(log=9, low=(34,)), of=Fse(log=8, low=(18,)), ml=Fse(log=9, low=(51,)), widest=True)
    assert wide.step_bits == 74, wide.step_bits
    decode_call([open_frame(601 + k, sequences(601 + k, 40 + k, MODES[k]), MODES[k]) for k in range(15)] + [wide])


def test_mixed_tables_in_one_wavefront():
    """Sixteen chains, sixteen combinations of table modes and accuracy logs, a hundred-odd sequences each."""
    decode_call([open_frame(700 + k, sequences(700 + k, 100 + 7 * k, MODES[k]), MODES[k]) for k in range(16)])


# what is done to the bit stream of one block (the kernel's status word it ends in: zstd_lanes.h)
DAMAGE = {
    "no_end_mark": lambda b: b[:-1] + b"\x00",            # 21: the last byte holds no set bit
    "shorter_than_the_initial_states": lambda b: b"\x01",  # 22: the end mark alone
    "runs_dry": lambda b: b[3:],                           # 23: the bits of the last sequences are missing
    "bits_left_over": lambda b: b"\x55\x55" + b,          # 24: sixteen bits nobody reads
}


@pytest.mark.parametrize("damage", list(DAMAGE))
@pytest.mark.parametrize("at", [0, 9, 15])
def test_a_malformed_block_among_valid_ones(damage, at):
    """Only the damaged chain's column fails, with the oracle's status; its fifteen neighbours in the wavefront are intact."""
    frames = []
    for k in range(16):
        tamper = (lambda name, b: DAMAGE[damage](b) if name == "bits" else b) if k == at else None
        modes = (P, P, P) if k == at else MODES[k]   # (predefined tables: 17 bits of initial states)
        frames.append(open_frame(800 + k, sequences(800 + k, 20 + 3 * k, modes), modes, tamper=tamper, check=k != at))
    (st, batch, col), cols, streams, total, bs = decode_call(frames, bad=(at,))
    assert st != 0 and col == at, (damage, at, st, batch, col)
    oc = G.oracle_column(cols[at], streams, "zstd", bs)
    ost = oc.status if oc.status != 0 else oc.next_batch(min(total // 8, 8192))["status"]
    assert st == ost, (damage, at, "status", st, "the oracle's", ost)
