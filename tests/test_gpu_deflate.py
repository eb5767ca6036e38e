"""GPU parity of the DEFLATE kernels on the hand-built streams of tests/test_deflate_cases.py (every one of them judged by
Python's zlib and by the oracle there, without a GPU) and on what zlib's less usual settings emit.

A DOUBLE column carries arbitrary bytes (see test_gpu_codecs.py): its DATA stream is the case's stream framed as ONE
compressed chunk, and an original chunk of zeros behind it pads the plain bytes to whole doubles.

Which kernels decode a chunk depends on how many chunks the call has (launch_chunk_decoders), so every case runs in two
call shapes: ALONE (the 256-thread token kernel, lz_exec_kernel) and next to a BALLAST column of more than
max(6 * CUs, 2048) small compressed chunks (the 64-thread token kernel, lz_exec_wave_kernel).  A valid chunk that the token
stage hands to the one-wavefront decoder still decodes, only slowly, so the parity tests cannot see it: a child process
runs every case under ORCGPU_DEBUG and reads the library's "deflate:" line to see what ran and what was deferred."""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import gpu_util as G
from test_deflate_cases import MALFORMED, ORACLE_ACCEPTS, VALID
from test_gpu_codecs import DATA, DOUBLE, frame, shapes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ["alone", "ballast"]
# what must decode: the cases zlib and the oracle agree on, and the ones only the oracle takes (a lone code that is not 1 bit long)
DECODES = dict(VALID)
DECODES.update({name: c[:2] for name, c in ORACLE_ACCEPTS.items()})

# Valid cases that the token stage hands to the one-wavefront decoder BY DESIGN: name -> why.  (None: keep it so.  The streams
# that do not self-synchronise must never be listed.)
DEFERRED_BY_DESIGN = {}


def chunk(block, original=False):
    h = (len(block) << 1) | int(original)
    assert h < (1 << 24)
    return np.frombuffer(bytes([h & 0xFF, (h >> 8) & 0xFF, (h >> 16) & 0xFF]) + block, dtype=np.uint8).copy()


def case_stream(stream, plain_len):
    pad = (-plain_len) % 8 if plain_len else 8
    return np.concatenate([chunk(stream), chunk(bytes(pad), original=True)]) if pad else chunk(stream), (plain_len + pad) // 8


def block_size_for(plain_len):
    b = 4096
    while b < plain_len:
        b *= 2
    return b


def ballast_chunks():
    """More chunks than either threshold of launch_chunk_decoders, from the device's CU count (the debug-line test below shows that
    the count was right: the ballast shape must have run the 64-thread kernels)."""
    import ctypes as C
    G.ctx()   # (the library has initialised the device)
    hip = C.CDLL("libamdhip64.so")
    cus = C.c_int(0)
    # hipDeviceAttributeMultiprocessorCount of hipDeviceAttribute_t, hip_runtime_api.h of ROCm 7.2 (torch does not see the device in
    # every test process, and the C ABI does not export the count).  Should a release renumber the enumeration, the debug-line test
    # fails: it checks the chunk counts and the kernels of both shapes.
    HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT = 63
    rc = hip.hipDeviceGetAttribute(C.byref(cus), HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT, 0)
    assert rc == 0 and 1 <= cus.value <= 4096, (rc, cus.value)
    return max(6 * cus.value, 2048) + 8


_ballast = {}


def ballast(rows):
    """A DATA stream of small plain chunks (64 bytes, more where `rows` doubles need it), each compressed on its own."""
    n = ballast_chunks()
    per = max(64, (rows * 8 + n - 1) // n + 7 & ~7)
    if per not in _ballast:
        raw = ((np.arange(n, dtype=np.uint32)[:, None] * 3 + (np.arange(per, dtype=np.uint32) % 8)[None, :]) & 0xFF).astype(np.uint8).tobytes()
        s = frame(raw, lambda b: (lambda c: c.compress(b) + c.flush())(zlib.compressobj(6, zlib.DEFLATED, -15)), per)
        assert len(s) < len(raw) // 2   # (compressed chunks, not original ones)
        _ballast[per] = s
    return _ballast[per]


def decode(stream, plain_len, shape, block_size):
    data, rows = case_stream(stream, plain_len)
    cols = [{"column_id": 1, "orc_type": DOUBLE, "encoding": 0}]
    streams = [(1, DATA, data)]
    if shape == "ballast":
        cols.append({"column_id": 2, "orc_type": DOUBLE, "encoding": 0})
        streams.append((2, DATA, ballast(rows)))
    res = G.gpu_decode(rows, cols, streams, compression="zlib", block_size=block_size)
    return res, cols, streams, rows


def values(res, ci):
    return b"".join(bytes(res.batch(b, ci)["values"]) for b in range(res.n_batches))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", list(DECODES))
def test_valid_case(name, shape):
    stream, plain = DECODES[name]
    bs = block_size_for(len(plain))
    res, cols, streams, rows = decode(stream, len(plain), shape, bs)
    assert res.status()[0] == 0, (name, shape, res.status())
    assert values(res, 0) == plain + bytes(rows * 8 - len(plain)), (name, shape, "not the model's bytes")
    for ci, c in enumerate(cols):
        G.assert_column_parity(res, ci, c, streams, rows, 8192, compression="zlib", block_size=bs, what=(name, shape, ci))
    res.free()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", list(MALFORMED))
def test_malformed_case(name, shape):
    """A non-zero status that is the oracle's; status 0 with wrong bytes, or a fault, is what this test exists for.  Beside the
    ballast column only the case's own column fails."""
    stream = MALFORMED[name]
    res, cols, streams, rows = decode(stream, 512, shape, 4096)
    st, batch, col = res.status()
    assert st != 0 and col == 0, (name, shape, res.status())
    oc = G.oracle_column(cols[0], streams, "zlib", 4096)
    ost = oc.status if oc.status != 0 else oc.next_batch(min(rows, 8192))["status"]
    assert st == ost, (name, shape, "status", st, "the oracle's", ost)
    for ci, c in enumerate(cols):
        G.assert_column_parity(res, ci, c, streams, rows, 8192, compression="zlib", block_size=4096, what=(name, shape, ci))
    res.free()


# ---- what zlib emits when asked for something else than level 6 -------------------------------------------------------------------
def _deflater(level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at_half=False):
    def compress(b):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
        if flush_at_half:
            return c.compress(b[:len(b) // 2]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(b[len(b) // 2:]) + c.flush()
        return c.compress(b) + c.flush()
    return compress


ENCODERS = {
    "level0": _deflater(0),                                  # stored blocks only
    "level1": _deflater(1),
    "level9": _deflater(9),
    "fixed": _deflater(6, strategy=zlib.Z_FIXED),            # fixed-Huffman blocks only
    "huffman_only": _deflater(6, strategy=zlib.Z_HUFFMAN_ONLY),
    "rle": _deflater(6, strategy=zlib.Z_RLE),                # distance 1 only
    "memlevel1": _deflater(6, mem=1),                        # many small dynamic blocks
    "full_flush_in_mid_chunk": _deflater(6, flush_at_half=True),   # an empty stored block and a reset window inside the chunk
}


def always_compressed(raw, compress, block):
    """Every block as a compressed chunk, also where that does not pay (level 0 never does: `frame` would store the block)."""
    return np.concatenate([chunk(compress(raw[p:p + block])) for p in range(0, len(raw), block)])


@pytest.mark.parametrize("block", [262144, 1000])
@pytest.mark.parametrize("enc", list(ENCODERS))
def test_real_encoders(enc, block):
    c = {"column_id": 1, "orc_type": DOUBLE, "encoding": 0}
    for name, raw in shapes(block).items():
        framings = [frame(raw, ENCODERS[enc], block)]
        if enc == "level0":
            framings.append(always_compressed(raw, ENCODERS[enc], block))
        for stream in framings:
            n = len(raw) // 8
            res = G.gpu_decode(n, [c], [(1, DATA, stream)], compression="zlib", block_size=block)
            assert res.status()[0] == 0, (enc, block, name, res.status())
            assert values(res, 0) == raw, (enc, block, name)
            G.assert_column_parity(res, 0, c, [(1, DATA, stream)], n, 8192, compression="zlib", block_size=block, what=(enc, block, name))
            res.free()


# ---- which kernels ran, and what the token stage handed to the one-wavefront decoder ------------------------------------------------
DEBUG_LINE = re.compile(r"\[orcgpu\] deflate: (\d+) chunks of (\d+) in the call, token stage (\d+) threads per chunk, execution (\d+) threads per chunk, "
                        r"(\d+) deferred to the serial decoder, (\d+) rejected by the execution kernel")


def child_main():
    """(in the child process) every case in both shapes; a marker line on stderr in front of each call's ORCGPU_DEBUG lines"""
    for shape in SHAPES:
        for kind, table in (("valid", DECODES), ("malformed", MALFORMED)):
            for name, case in table.items():
                stream, plain_len, bs = (case[0], len(case[1]), block_size_for(len(case[1]))) if kind == "valid" else (case, 512, 4096)
                sys.stderr.write("\nCASE %s %s %s\n" % (kind, name, shape))
                sys.stderr.flush()
                res = decode(stream, plain_len, shape, bs)[0]
                sys.stderr.write("\nSTATUS %d\n" % res.status()[0])
                sys.stderr.flush()
                res.free()
    sys.stderr.write("\nCASE end end end\n")


def test_the_debug_line_names_the_kernels_and_no_valid_case_is_deferred():
    env = {k: v for k, v in os.environ.items() if not k.startswith("ORCGPU_")}
    env["ORCGPU_DEBUG"] = "1"
    code = "import os, sys; sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests')); import test_gpu_deflate as T; T.child_main()" % (ROOT, ROOT)
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1500)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == 0, err[-3000:]
    calls, cur = {}, None
    for line in err.splitlines():
        if line.startswith("CASE "):
            cur = tuple(line.split()[1:4])
            calls[cur] = {"lines": [], "status": None}
        elif line.startswith("STATUS ") and cur:
            calls[cur]["status"] = int(line.split()[1])
        elif cur:
            m = DEBUG_LINE.search(line)
            if m:
                calls[cur]["lines"].append(tuple(int(x) for x in m.groups()))
    assert ("end", "end", "end") in calls
    want_threads = {"alone": (256, 256), "ballast": (64, 64)}   # (token kernel, execution kernel) threads per chunk
    n_ballast = ballast_chunks()
    wrong_shape, deferred_valid, undeferred_malformed, wrong_runs = [], [], [], []
    for shape in SHAPES:
        for kind, table in (("valid", DECODES), ("malformed", MALFORMED)):
            for name in table:
                c = calls[(kind, name, shape)]
                assert c["lines"], (kind, name, shape, "no deflate line")
                # the call's chunks: the case's one, the ballast column's, and the original chunk that pads the case to whole doubles
                plain_len = len(table[name][1]) if kind == "valid" else 512
                want_deflate = 1 + (n_ballast if shape == "ballast" else 0)
                want_chunks = want_deflate + (1 if plain_len % 8 or not plain_len else 0)
                for n_deflate, n_chunks, t_threads, x_threads, deferred, rejected in c["lines"]:
                    if (t_threads, x_threads) != want_threads[shape] or (n_deflate, n_chunks) != (want_deflate, want_chunks):
                        wrong_shape.append((name, shape, t_threads, x_threads, n_deflate, n_chunks, "expected", want_threads[shape], want_deflate, want_chunks))
                    if kind == "valid":
                        if (deferred or rejected) and name not in DEFERRED_BY_DESIGN:
                            deferred_valid.append((name, shape, deferred, rejected))
                    elif deferred + rejected != 1:
                        # its one chunk: left to the one-wavefront decoder (a bad header, a token that cannot be, the end of the input), or
                        # rejected by the execution kernel (a distance beyond the start, output beyond the slot); and no other chunk
                        undeferred_malformed.append((name, shape, deferred, rejected))
                # (a failed chunk gets the 4 MiB head-room and the call runs once more: two lines)
                if (c["status"] == 0, len(c["lines"])) != ((True, 1) if kind == "valid" else (False, 2)):
                    wrong_runs.append((kind, name, shape, c["status"], len(c["lines"])))
    print("deflate debug lines: %d calls; wrong shape %d, valid deferred %d, malformed not stopped %d, wrong runs %d"
          % (len(calls) - 1, len(wrong_shape), len(deferred_valid), len(undeferred_malformed), len(wrong_runs)))
    assert not wrong_shape, ("calls that did not run the kernels or the chunks they were built for", wrong_shape[:8])
    assert not deferred_valid, ("valid chunks the token stage gave up on, or the execution kernel rejected", deferred_valid)
    assert not undeferred_malformed, ("malformed chunks that were not stopped by exactly one of the two stages", undeferred_malformed[:20])
    assert not wrong_runs, ("status / number of runs", wrong_runs[:20])
    for name in DEFERRED_BY_DESIGN:
        assert not name.startswith("nonsync"), name
