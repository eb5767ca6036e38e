"""The HIP String / Binary finishers (device/string_kernels.hip: string_lens_body, batch_offsets_body, utf8_validate_body,
copy_validate_body, utf8_boundaries_body, dict_offsets_body, the four gather paths of dict_emit_kernel, dict_keys_kernel) on the
hand-built tables of tests/test_string_cases.py.  Every case is checked twice: against the expectation written next to it -- offsets
and value bytes bit for bit, or the error kind and the failing batch with every batch in front intact -- AND against the CPU
oracle (G.assert_column_parity).

A failing column ends the stripe (one status per result), so every failing case is a call of its own; valid cases of one row
count are the columns of one call."""
import numpy as np
import pytest

import gpu_util as G
import string_model as M
import test_string_cases as T
from orc_rust_amd import gen

pytestmark = pytest.mark.gpu

DICTIONARY_UTF8 = 27  # arrow_target: int32 keys and the stripe's dictionary (dict_keys_kernel)


def packed(b, compression):
    return b if compression == "none" else gen.compress_stream(bytes(b), compression, 64)


def column_of(case, cid, orc_type=None, target=0):
    c = dict(case["column"], column_id=cid)
    if orc_type is not None and c["orc_type"] != T.BINARY:
        c["orc_type"] = orc_type
    if target:
        c["arrow_target"] = target
    return c


def streams_of(case, cid, compression="none"):
    return [(cid, kind, packed(b, compression)) for _, kind, b in case["streams"]]


def assert_batches(res, ci, front, what):
    """the batches in `front`, offsets and value bytes, bit for bit"""
    for b, (offsets, values) in enumerate(front):
        got = res.batch(b, ci)
        assert got["offsets"].tolist() == offsets, (what, "offsets of batch", b)
        assert got["values"] == values, (what, "values of batch", b, len(got["values"]), len(values))


def run_valid(cases, batch, orc_type=None, compression="none"):
    """cases of one row count, a column each, in one call"""
    n_rows = cases[0]["n_rows"]
    assert all(c["n_rows"] == n_rows for c in cases)
    kw = {} if compression == "none" else {"compression": compression, "block_size": 64}
    cols = [column_of(c, i + 1, orc_type) for i, c in enumerate(cases)]
    streams = [s for i, c in enumerate(cases) for s in streams_of(c, i + 1, compression)]
    res = G.gpu_decode(n_rows, cols, streams, batch_size=batch, **kw)
    assert res.status()[0] == 0, ([c["name"] for c in cases], batch, res.status())
    for ci, case in enumerate(cases):
        what = (case["name"], batch, orc_type, compression)
        front, failure = case["want"](batch)
        assert failure is None and res.n_batches == len(front), what
        assert_batches(res, ci, front, what)
        G.assert_column_parity(res, ci, cols[ci], streams, n_rows, batch, what=what, **kw)
    res.free()


def by_rows(cases, batch):
    groups = {}
    for c in cases:
        if batch in c["batches"]:
            groups.setdefault(c["n_rows"], []).append(c)
    return groups.values()


def run_failing(case, batch, orc_type=None, target=0):
    """a call of its own: the status word names the kind and the failing batch, every batch in front is intact"""
    col, streams = column_of(case, 1, orc_type, target), streams_of(case, 1)
    what = (case["name"], batch, orc_type, target)
    front, (kind, fb) = case["want"](batch)
    res = G.gpu_decode(case["n_rows"], [col], streams, batch_size=batch)
    st, gbatch, gcol = res.status()
    # (a dictionary that cannot be built fails the column before any batch: the status word says batch 0)
    assert (st, gbatch, gcol) == (kind, max(fb, 0), 0), (what, "gpu", (st, gbatch), "want", (kind, fb))
    if target:
        assert_keys(res, case, batch, len(front), what)
    else:
        assert_batches(res, 0, front, what)
        G.assert_column_parity(res, 0, col, streams, case["n_rows"], batch, what=what)
    res.free()


def cases_of(table, prefix):
    return [c for name, c in table.items() if name.startswith(prefix)]


# ---- direct String and Binary -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orc_type", [T.STRING, T.VARCHAR, T.CHAR])
def test_valid_direct_cases(orc_type):
    """every valid case at every batch size of its own; as Varchar and Char the same bytes (the Binary cases stay Binary)"""
    cases = [c for c in T.VALID.values() if orc_type == T.STRING or c["utf8"]]
    assert len(cases) >= 25
    for batch in sorted({b for c in cases for b in c["batches"]}):
        for group in by_rows(cases, batch):
            run_valid(group, batch, orc_type)


DIRECT_GROUPS = ("utf8/", "boundary/", "batch boundary/", "row boundary/", "ascii/", "short DATA/", "two errors/", "one batch/", "sums/")


def test_every_malformed_direct_case_is_in_a_group():
    assert all(name.startswith(DIRECT_GROUPS) for name in T.MALFORMED)


@pytest.mark.parametrize("group", DIRECT_GROUPS)
def test_malformed_direct_cases(group):
    cases = cases_of(T.MALFORMED, group)
    assert cases
    for case in cases:
        for batch in case["batches"]:
            run_failing(case, batch)


def test_malformed_direct_cases_as_varchar_and_char():
    for name in ("utf8/ED A0 80", "utf8/F4 90 80 80 inside a row", "batch boundary/2 of 4 bytes in front", "sums/the sum is 2^31, batch 2", "sums/-1 next to 2^31, batch 2"):
        case = T.MALFORMED[name]
        for orc_type in (T.VARCHAR, T.CHAR):
            run_failing(case, case["batches"][0], orc_type)


# ---- dictionaries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(T.SHAPES))
def test_dictionary_shapes(shape):
    """each gather path and key width, rows with and without a PRESENT stream in one call, at batch sizes 8192, 999 and 1; as Varchar
    and Char once more"""
    cases = [T.DICT_VALID[shape], T.DICT_VALID[shape + ", with nulls"]]
    for batch in T.DICT_BATCHES:
        run_valid(cases, batch)
    run_valid(cases, 999, T.VARCHAR)
    run_valid(cases, 8192, T.CHAR)


def test_other_valid_dictionary_cases():
    names = [n for n in T.DICT_VALID if n.split(", with nulls")[0] not in T.SHAPES]
    assert len(names) >= 4
    for name in names:
        case = T.DICT_VALID[name]
        for batch in case["batches"]:
            run_valid([case], batch)


@pytest.mark.parametrize("group", ["keys/", "dictionary/"])
def test_malformed_dictionary_cases(group):
    cases = cases_of(T.DICT_MALFORMED, group)
    assert len(cases) >= 10
    for case in cases:
        for batch in case["batches"]:
            run_failing(case, batch)


# ---- Arrow Dictionary output: the keys stay keys (dict_keys_kernel) ---------------------------------------------------------------
def assert_keys(res, case, batch, n_batches, what):
    """the first n_batches batches: one int32 key per row, 0 in a null row; the dictionary the file's, entry for entry"""
    flags = case["present"] or [1] * len(case["keys"])
    it = iter(case["keys"])
    want = [next(it) if f else 0 for f in flags[:n_batches * batch]]
    for b in range(n_batches):
        got = res.batch(b, 0)
        assert got["offsets"] is None, what
        assert np.frombuffer(got["values"], dtype=np.int32).tolist() == want[b * batch:(b + 1) * batch], (what, "keys of batch", b)
        bits = None if got["validity"] is None else [bool(got["validity"][i >> 3] >> (i & 7) & 1) for i in range(got["length"])]
        rows = flags[b * batch:(b + 1) * batch]
        assert bits == (None if all(rows) else [bool(f) for f in rows]), (what, "validity of batch", b)
    if n_batches:
        model = M.byte_batch(case["dict_lengths"][:case["dictionary_size"]], case["dict_data"], 0, True)
        offsets, blob = res.dictionary(0)
        assert (offsets.tolist(), blob) == (model[0], model[1]), (what, "dictionary")
        assert [blob[offsets[k]:offsets[k + 1]] for k in range(len(offsets) - 1)] == case["entries"], (what, "entries")


@pytest.mark.parametrize("shape", list(T.SHAPES))
def test_dictionary_shapes_as_arrow_dictionary(shape):
    for name in (shape, shape + ", with nulls"):
        case = T.DICT_VALID[name]
        for batch in (8192, 999):
            res = G.gpu_decode(case["n_rows"], [column_of(case, 1, target=DICTIONARY_UTF8)], streams_of(case, 1), batch_size=batch)
            assert res.status()[0] == 0, (name, batch, res.status())
            n_batches = (case["n_rows"] + batch - 1) // batch
            assert res.n_batches == n_batches
            assert_keys(res, case, batch, n_batches, (name, batch))
            # the keys through the dictionary are the rows the case was written from
            offsets, blob = res.dictionary(0)
            keys = np.concatenate([np.frombuffer(res.batch(b, 0)["values"], dtype=np.int32) for b in range(n_batches)])
            flags = case["present"] or [1] * case["n_rows"]
            assert [blob[offsets[k]:offsets[k + 1]] if f else None for k, f in zip(keys, flags)] == case["rows"], (name, batch)
            res.free()


def test_malformed_dictionary_cases_as_arrow_dictionary():
    """a key that is none, a dictionary that cannot be built: the same kind, the same batch"""
    cases = list(T.DICT_MALFORMED.values())
    assert len(cases) >= 60
    for case in cases:
        for batch in case["batches"]:
            run_failing(case, batch, target=DICTIONARY_UTF8)


# ---- the streams in compression chunks of 64 bytes ----------------------------------------------------------------------------------
def test_streams_in_zstd_chunks_of_64_bytes():
    """the DATA bytes of a direct column are then decompressed into the result's value buffer (and only checked there), a
    dictionary's bytes into the workspace"""
    for table, names in ((T.VALID, ("boundary/16", "boundary/4096", "lengths/0 to 4097, with nulls", "lengths/0 to 4097, Binary")),
                         (T.DICT_VALID, ("100 entries of 33 bytes", "100 entries of 33 bytes, with nulls", "an entry of 64 bytes, with nulls"))):
        for name in names:
            case = table[name]
            for batch in case["batches"][:2]:
                run_valid([case], batch, compression="zstd")
