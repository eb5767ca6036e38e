"""A staged stream carries its part of the decompressors' tables (orcgpu_decomp_plan.inc: built once by orcgpu_stage_stripe); a
decode call merges the parts of its streams and rebases them.  Small lineitem stripes (20 000 rows, all 16 columns, Zstandard in
256 KiB and in 4 KiB chunks: one block and dozens of blocks per stream) decoded alone, two and three to a call, repeatedly and
with changing partners, in both Zstandard modes (one wavefront / one lane per block: sequence scratch of 12 / 8 bytes): every
Arrow buffer must equal the one the oracle vouched for.  Also a stripe staged under a row selection of two row groups (chunk
lists that are subsets, entry points inside chunks), and staging again after a stripe was freed."""
import numpy as np
import pytest

import gpu_util as G
from orc_rust_amd.gen import workloads as W

pytestmark = pytest.mark.gpu

ROWS = 20_000


def snapshot(res, n_cols):
    return [[res.batch(b, ci) for ci in range(n_cols)] for b in range(res.n_batches)]


def same(ref, got, what):
    assert len(ref) == len(got), what
    for b, (rb, gb) in enumerate(zip(ref, got)):
        for ci, (r1, g1) in enumerate(zip(rb, gb)):
            assert r1["values"] == g1["values"] and r1["validity"] == g1["validity"] and r1["null_count"] == g1["null_count"], (what, b, ci)
            assert (r1["offsets"] is None) == (g1["offsets"] is None) and (r1["offsets"] is None or np.array_equal(r1["offsets"], g1["offsets"])), (what, b, ci)


@pytest.fixture(scope="module", params=[262144, 4096])
def data(request):
    """Three stripes and, per stripe, the buffers of a decode on its own that the oracle agreed with column by column."""
    block = request.param
    table = W.lineitem_table(3 * ROWS)
    stripes = [W.lineitem_stripe(table, k * ROWS, (k + 1) * ROWS, "zstd", block_size=block) for k in range(3)]
    refs = []
    for n, cols, streams, expect in stripes:
        res = G.gpu_decode(n, cols, streams, compression="zstd", block_size=block)
        assert res.status()[0] == 0, res.status()
        W.check_result(res, cols, expect)
        for ci, c in enumerate(cols):
            G.assert_column_parity(res, ci, c, streams, n, 8192, compression="zstd", block_size=block, what=("reference", block, c["name"]))
        refs.append(snapshot(res, len(cols)))
        res.free()
    return block, stripes, refs


def stage(c, stripe, block):
    n, cols, streams, _ = stripe
    return c.stage(n, streams, cols, compression="zstd", block_size=block)


def decode_and_compare(c, staged, which, refs, n_cols, what, results=None):
    results = c.decode([staged[k] for k in which], results)
    for k, res in zip(which, results):
        assert res.status()[0] == 0, (what, k, res.status())
        same(refs[k], snapshot(res, n_cols), (what, which, k))
    return results


@pytest.mark.parametrize("mode", ["0", "1"])
def test_stripes_alone_and_two_and_three_to_a_call(monkeypatch, data, mode):
    block, stripes, refs = data
    monkeypatch.setenv("ORCGPU_ZSTD_LANES", mode)
    c = G.ctx()
    staged = [stage(c, s, block) for s in stripes]
    n_cols = len(stripes[0][1])
    try:
        for which in ([0, 1], [0, 1, 2], [0], [1], [2]):
            for r in decode_and_compare(c, staged, which, refs, n_cols, ("call", block, mode)):
                r.free()
    finally:
        for s in staged:
            s.free()


def test_a_call_leaves_the_staged_tables_as_they_were(monkeypatch, data):
    """The same staged stripe twice (into the same results), then with a partner behind it, with another in front of it, and
    in the other Zstandard mode: its tables are rebased into the call's copy, never in place."""
    block, stripes, refs = data
    c = G.ctx()
    staged = [stage(c, s, block) for s in stripes]
    n_cols = len(stripes[0][1])
    try:
        monkeypatch.setenv("ORCGPU_ZSTD_LANES", "1")
        results = decode_and_compare(c, staged, [0], refs, n_cols, "first")
        results = decode_and_compare(c, staged, [0], refs, n_cols, "second", results)
        for r in results:
            r.free()
        for which, mode in (([0, 2], "1"), ([1, 0], "0"), ([0], "0"), ([2, 0, 1], "1"), ([0], "1")):
            monkeypatch.setenv("ORCGPU_ZSTD_LANES", mode)
            for r in decode_and_compare(c, staged, which, refs, n_cols, ("partners", mode)):
                r.free()
    finally:
        for s in staged:
            s.free()


def test_free_a_staged_stripe_and_stage_another(data):
    block, stripes, refs = data
    c = G.ctx()
    n_cols = len(stripes[0][1])
    for k in (0, 1, 0, 2):  # (the freed stripe's arena goes back to the pool: the next one takes it)
        s = stage(c, stripes[k], block)
        try:
            res = c.decode([s])[0]
            assert res.status()[0] == 0, res.status()
            same(refs[k], snapshot(res, n_cols), ("staged again", k))
            res.free()
        finally:
            s.free()


@pytest.mark.parametrize("mode", ["0", "1"])
def test_a_stripe_staged_under_a_row_selection_of_two_row_groups(monkeypatch, tmp_path, mode):
    """The reader stages only the row groups a selection touches, every stream from the entry point its ROW_INDEX names: chunk
    lists that are subsets of the streams' chunks.  Two row groups of one Zstandard stripe (64 KiB chunks, stride 1000) against
    the table the file was written from and against the whole-stripe read (test_gpu_rowgroups.check)."""
    import test_gpu_rowgroups as R
    monkeypatch.setenv("ORCGPU_ZSTD_LANES", mode)
    table = R.make_table(ROWS, seed=31)
    path = R.write(tmp_path, table, "two_groups.orc", compression="zstd", compression_block_size=65536, row_index_stride=1000, stripe_size=64 << 20,
                   dictionary_key_size_threshold=0.5)
    assert len(R.stripe_rows(path)) == 1
    sel = [R.S(3_400), R.K(200), R.S(8_000), R.K(300), R.S(ROWS - 11_900)]
    g_read, g_total = R.check(table, path, sel)
    assert (g_read, g_total) == (2, 20), (g_read, g_total)
