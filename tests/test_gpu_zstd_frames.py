"""GPU parity of the Zstandard kernels on the hand-built frames of tests/test_zstd_cases.py (every one of them judged by libzstd
and by the oracle there, without a GPU).

A DOUBLE column carries arbitrary bytes (see test_gpu_codecs.py): its DATA stream is the case's payload framed as ONE
compressed chunk, and an original chunk of zeros behind it pads the plain bytes to whole doubles, as in test_gpu_deflate.py.
Every case runs in the two Zstandard paths the library has (ORCGPU_ZSTD_LANES=0: a wavefront per block; =1: the table-scale
kernels of device/zstd_lanes.h), the valid table once more with the literals kernel in front of the sequences kernel
(ORCGPU_ZSTD_LIT_ASIDE=0), and all valid cases together as the columns of one call.

Status 0 with wrong bytes is what this file exists to catch.
"""
import pytest

import gpu_util as G
from test_gpu_codecs import DATA, DOUBLE
from test_gpu_deflate import block_size_for, case_stream, values
from test_zstd_cases import MALFORMED, RFC_FOLLOWED, VALID

pytestmark = pytest.mark.gpu

GOOD = VALID
BAD = dict(MALFORMED)
BAD.update({n: c[0] for n, c in RFC_FOLLOWED.items()})   # refused like the oracle refuses them
COL = {"column_id": 1, "orc_type": DOUBLE, "encoding": 0}


@pytest.fixture(params=["0", "1"])
def lanes(request, monkeypatch):
    monkeypatch.setenv("ORCGPU_ZSTD_LANES", request.param)
    return request.param


def check_valid(name, what):
    payload, plain = GOOD[name]
    bs = block_size_for(len(plain))
    data, rows = case_stream(payload, len(plain))
    streams = [(1, DATA, data)]
    res = G.gpu_decode(rows, [COL], streams, compression="zstd", block_size=bs)
    try:
        assert res.status()[0] == 0, (name, what, res.status())
        assert values(res, 0) == plain + bytes(rows * 8 - len(plain)), (name, what, "not the model's bytes")
        G.assert_column_parity(res, 0, COL, streams, rows, 8192, compression="zstd", block_size=bs, what=(name, what))
    finally:
        res.free()


@pytest.mark.parametrize("name", list(GOOD))
def test_valid_case(name, lanes):
    check_valid(name, ("lanes", lanes))


@pytest.mark.parametrize("name", list(GOOD))
def test_valid_case_with_the_literals_kernel_in_front(name, monkeypatch):
    monkeypatch.setenv("ORCGPU_ZSTD_LANES", "1")
    monkeypatch.setenv("ORCGPU_ZSTD_LIT_ASIDE", "0")
    check_valid(name, "literals in front")


@pytest.mark.parametrize("name", list(BAD))
def test_malformed_case(name, lanes):
    """A non-zero status that is the oracle's; status 0 with wrong bytes, or a fault, is what this test exists for."""
    data, rows = case_stream(BAD[name], 512)
    streams = [(1, DATA, data)]
    res = G.gpu_decode(rows, [COL], streams, compression="zstd", block_size=4096)
    try:
        st, batch, col = res.status()
        assert st != 0 and col == 0, (name, lanes, res.status())
        oc = G.oracle_column(COL, streams, "zstd", 4096)
        ost = oc.status if oc.status != 0 else oc.next_batch(min(rows, 8192))["status"]
        assert st == ost, (name, lanes, "status", st, "the oracle's", ost)
        G.assert_column_parity(res, 0, COL, streams, rows, 8192, compression="zstd", block_size=4096, what=(name, lanes))
    finally:
        res.free()


# rows = the shortest column's, so one call of ALL cases compares eight bytes of each (the empty-bodied ones carry eight bytes of
# padding).  The same call is therefore made again per size class -- columns whose row counts lie within a factor of four --, which
# compares at least a quarter of every column behind its start.
def size_classes():
    classes = {}
    for name, (payload, plain) in GOOD.items():
        classes.setdefault((max(len(plain), 8) // 8).bit_length() // 2, []).append(name)
    return [("all", list(GOOD))] + [("rows_4^%d" % k, v) for k, v in sorted(classes.items()) if len(v) > 1]


@pytest.mark.parametrize("names", [v for _, v in size_classes()], ids=[k for k, _ in size_classes()])
def test_valid_cases_as_the_columns_of_one_call(names, lanes):
    """Every frame its own column, rows = the shortest: chains of very different lengths and table modes share wavefronts in the
    lanes kernel."""
    bs = block_size_for(max(len(GOOD[n][1]) for n in names))
    cols, streams, rows = [], [], []
    for k, (name, (payload, plain)) in enumerate((n, GOOD[n]) for n in names):
        data, n = case_stream(payload, len(plain))
        cols.append({"column_id": k + 1, "orc_type": DOUBLE, "encoding": 0})
        streams.append((k + 1, DATA, data))
        rows.append(n)
    n = min(rows)
    res = G.gpu_decode(n, cols, streams, compression="zstd", block_size=bs)
    try:
        assert res.status()[0] == 0, res.status()
        for ci, (name, (payload, plain)) in enumerate((n_, GOOD[n_]) for n_ in names):
            want = (plain + bytes(8))[:n * 8]
            assert values(res, ci) == want, (name, lanes, "not the model's bytes")
            G.assert_column_parity(res, ci, cols[ci], streams, n, 8192, compression="zstd", block_size=bs, what=("one call", lanes, name))
    finally:
        res.free()
