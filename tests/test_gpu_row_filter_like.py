"""SQL LIKE in the row filter on the GPU (ORCGPU_PRED_LIKE: filter_like_kernel in device/filter_kernels.hip, the patterns compiled
by orcgpu_filter_plan.inc) against the model of tests/like_model.py: files written here with pyarrow.orc, read back with
pyarrow.orc, filtered per stripe by the model and rebatched -- the reader must hand out exactly those batches."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import filter_model as FM
import like_model as LM
import selection_model as M
from orc_rust_amd import capi, predicate as PR
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

pytestmark = pytest.mark.gpu

N = 4097
BATCH_SIZES = (64, 1000)
COMPRESSIONS = ("uncompressed", "zlib")
MISMATCHED, UNSUPPORTED, INVALID = 6, 7, 101
_CTX = None
_FILES = {}
_TABLE = None
_MASKS = {}


def ctx():
    global _CTX
    if _CTX is None:
        _CTX = capi.Context()
    return _CTX


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    capi.load()
    return tmp_path_factory.mktemp("row_filter_like")


def random_text(rng, n_max):
    return "".join("abcé"[k] for k in rng.integers(0, 4, int(rng.integers(0, n_max))))


def make_table():
    """id; s: the corner values cycled, mixed with random text over four letters (short for the lane per value, long for the
    wavefront), 20 % nulls; v: an Int64 with nulls; bin: a Binary column for the refusal."""
    global _TABLE
    if _TABLE is None:
        rng = np.random.default_rng(11)
        s = []
        for k in range(N):
            r = k % 3
            s.append(LM.VALUES[(k // 3) % len(LM.VALUES)] if r == 0 else random_text(rng, 12 if r == 1 else 90))
        null = rng.random(N) < 0.2
        s = [None if m else x for x, m in zip(s, null)]
        v = [None if m else int(x) for x, m in zip(rng.integers(-50, 50, N), rng.random(N) < 0.2)]
        _TABLE = pa.table({"id": pa.array(np.arange(N, dtype=np.int64)), "s": pa.array(s, pa.string()), "v": pa.array(v, pa.int64()),
                           "bin": pa.array([None if x is None else x.encode() for x in s], pa.binary())})
    return _TABLE


def orc_file(tmpdir, compression):
    """(path, the file's rows as pyarrow reads them, rows per stripe)"""
    if compression not in _FILES:
        path = str(tmpdir / ("like_%s.orc" % compression))
        orc.write_table(make_table(), path, compression=compression, stripe_size=1024, row_index_stride=1000,
                        batch_size=1500 if compression == "uncompressed" else 300)
        f = orc.ORCFile(path)
        rows = [f.read_stripe(i).num_rows for i in range(f.nstripes)]
        assert f.nstripes >= 2, rows
        _FILES[compression] = (path, f.read(), rows)
    return _FILES[compression]


# ---- the model: LIKE leaves by tests/like_model.py, everything else by tests/filter_model.py ----
def evaluate(pred, table):
    n = table.num_rows
    if pred.op == PR.LIKE:
        pattern = pred.value.value
        got = LM.like_column(table.column(pred.column).to_pylist(), pattern.decode() if isinstance(pattern, bytes) else pattern, pred.escape)
        return np.array([g is True for g in got], bool).reshape(n), np.array([g is False for g in got], bool).reshape(n)
    if pred.op == PR.AND:
        acc = (np.ones(n, bool), np.zeros(n, bool))
        for c in pred.children:
            acc = FM.and3(acc, evaluate(c, table))
        return acc
    if pred.op == PR.OR:
        acc = (np.zeros(n, bool), np.ones(n, bool))
        for c in pred.children:
            acc = FM.or3(acc, evaluate(c, table))
        return acc
    if pred.op == PR.NOT:
        return FM.not3(evaluate(pred.children[0], table))
    return FM.evaluate(pred, table)


def expected_batches(table, mask, stripe_rows, batch_size, selection_batches=None):
    out, base = [], 0
    for k, n in enumerate(stripe_rows):
        idx = np.arange(base, base + n)
        if selection_batches is not None and selection_batches[k] is not None:
            idx = np.concatenate([np.arange(base + s, base + s + m) for s, m in selection_batches[k]] or [np.arange(0)]).astype(np.int64)
        kept = table.take(pa.array(idx[mask[idx]]))
        out += FM.rebatch(kept, [kept.num_rows], batch_size)
        base += n
    return out


def read(path, pred, batch_size=1000, prune=False, prefetch=0, selection=None, device=False, names=None, dictionary=None):
    b = ArrowReaderBuilder.try_new(path, ctx()).with_batch_size(batch_size).with_prefetch(prefetch)
    if names is not None:
        b = b.with_projection(names)
    if dictionary is not None:
        b = b.with_dictionary_columns(dictionary)
    if selection is not None:
        b = b.with_row_selection(selection)
    b = b.with_row_filter(pred, prune=prune)
    if device:
        b = b.with_device_output()
    r = b.build()
    try:
        batches = [x.to_pyarrow() for x in r] if device else list(r)
        return batches, r.filter_rows(), r.row_groups()
    finally:
        r.close()


def check(path, table, rows, pred, batch_size, mask=None, selection=None, **kw):
    if mask is None:
        mask = evaluate(pred, table)[0]
    sel_batches = M.file_batches(selection, rows, batch_size) if selection is not None else None
    want = expected_batches(table, mask, rows, batch_size, sel_batches)
    got, (seen, kept), groups = read(path, pred, batch_size=batch_size, selection=selection, **kw)
    what = (os.path.basename(path), batch_size, kw)
    assert [b.num_rows for b in got] == [w.num_rows for w in want], what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.num_rows == w.num_rows and g.schema.names == w.schema.names, what
        g.validate(full=True)
        for name in w.schema.names:
            assert g.column(name).cast(w.column(name).type).equals(w.column(name).combine_chunks()), what + (k, name)
    assert kept == sum(w.num_rows for w in want), what
    return got, (seen, kept), groups


def all_patterns():
    return [(p, "\\") for p in LM.PATTERNS] + LM.ESCAPED


def like_mask(table, pattern, escape):
    """(TRUE rows, FALSE rows) of the LIKE leaf over the whole table, computed once"""
    key = (pattern, escape)
    if key not in _MASKS:
        _MASKS[key] = evaluate(P.like("s", pattern, escape), table)
    return _MASKS[key]


def test_the_inputs_tell_a_matcher_that_answers_all_or_none():
    """On the CPU, from the model alone: every pattern keeps a row and drops a non-null row (but for the keep-all patterns, and
    the empty pattern keeps only empty values), so neither "all" nor "none" can pass the comparisons below."""
    table = make_table()
    values = table.column("s").to_pylist()
    assert 0.15 < sum(v is None for v in values) / N < 0.25
    for pattern, escape in all_patterns():
        t, f = like_mask(table, pattern, escape)
        assert not (t & f).any() and int(t.sum() + f.sum()) == sum(v is not None for v in values)
        if pattern in LM.KEEP_ALL:
            assert f.sum() == 0 and t.sum() > 0, pattern
        else:
            assert t.sum() > 0 and f.sum() > 0, (pattern, int(t.sum()), int(f.sum()))
        if pattern == "":
            assert all(values[k] == "" for k in np.flatnonzero(t))
    # long values take the wavefront path and short ones the lane path, on both sides of every answer
    for pattern in ("%" + LM.NEEDLE + "%", "%a%b%a%b%a%", "%c_abc"):
        t, f = like_mask(table, pattern, "\\")
        for side in (t, f):
            lens = [len(values[k].encode()) for k in np.flatnonzero(side)]
            assert min(lens) <= 32 and max(lens) > 32, pattern


@pytest.mark.parametrize("compression", COMPRESSIONS)
@pytest.mark.parametrize("batch_size", BATCH_SIZES)
def test_every_pattern_against_the_model(tmpdir, batch_size, compression):
    path, table, rows = orc_file(tmpdir, compression)
    for pattern, escape in all_patterns():
        t, f = like_mask(table, pattern, escape)
        _, (seen, kept), _ = check(path, table, rows, P.like("s", pattern, escape), batch_size, mask=t)
        assert (seen, kept) == (N, int(t.sum())), pattern
        _, (seen, kept), _ = check(path, table, rows, P.not_like("s", pattern, escape), batch_size, mask=f)
        assert (seen, kept) == (N, int(f.sum())), pattern  # a null row is dropped either way
    # bytes patterns, the conveniences, the NULL pattern
    check(path, table, rows, P.like("s", "%é_b%".encode()), batch_size)
    check(path, table, rows, P.starts_with("s", "a%"), batch_size)
    check(path, table, rows, P.ends_with("s", "_b"), batch_size)
    check(path, table, rows, P.contains("s", "\\"), batch_size)
    for pred in (P.like("s", None), P.not_like("s", None)):
        got, (seen, kept), _ = check(path, table, rows, pred, batch_size)
        assert got == [] and (seen, kept) == (N, 0)


def test_inside_and_or_with_an_integer_leaf_and_several_like_leaves(tmpdir):
    path, table, rows = orc_file(tmpdir, "uncompressed")
    a, b, keep_all = P.like("s", "%a%a%"), P.like("s", "%" + LM.NEEDLE + "%"), P.like("s", "%")
    preds = [P.and_([a, P.gt("v", V.Int64(0))]), P.or_([b, P.lt("v", V.Int64(-40))]), P.and_([P.not_(a), P.or_([b, P.is_null("v")])]),
             P.or_([P.and_([a, b]), P.not_(keep_all)]), P.and_([keep_all, P.not_(b), P.gte("id", V.Int64(63))]),
             P.not_(P.or_([a, b, P.like("s", "h_%"), P.like("s", "%c_abc"), P.eq("v", V.Int64(None))]))]
    for pred in preds:
        for batch_size in BATCH_SIZES:
            _, (seen, kept), _ = check(path, table, rows, pred, batch_size, prefetch=2 if batch_size == 64 else 0)
            assert 0 < kept < N or pred is preds[-1]


@pytest.mark.parametrize("compression", COMPRESSIONS)
def test_under_a_row_selection_with_pruning_and_with_device_output(tmpdir, compression):
    path, table, rows = orc_file(tmpdir, compression)
    selections = [[(5, True), (60, False), (1000, True), (700, False), (2000, True), (300, False)], [(1, False), (4095, True), (1, False)],
                  [(100, True), (1, False), (63, True), (65, False)]]
    for pattern in ("%aab", "ab%ba", "%a%a%", "_é", "%", "%c_abc"):
        t, f = like_mask(table, pattern, "\\")
        for batch_size in BATCH_SIZES:
            for sel in selections:
                check(path, table, rows, P.like("s", pattern, "\\"), batch_size, mask=t, selection=sel)
            check(path, table, rows, P.like("s", pattern, "\\"), batch_size, mask=t, prune=True, prefetch=2)
            check(path, table, rows, P.like("s", pattern, "\\"), batch_size, mask=t, device=True)
            check(path, table, rows, P.not_like("s", pattern, "\\"), batch_size, mask=f, device=True, selection=selections[0])


def test_pruning_is_sound_and_reads_fewer_row_groups(tmpdir):
    """A sorted string column with row groups of 1000 rows: a prefix pattern reads fewer row groups with prune=True and keeps
    the same rows; no pattern ever loses a row the model keeps."""
    rng = np.random.default_rng(5)
    words = sorted(random_text(rng, 10) + "x" for _ in range(6000))
    table = pa.table({"id": pa.array(np.arange(6000, dtype=np.int64)), "s": pa.array(words, pa.string())})
    path = str(tmpdir / "sorted.orc")
    orc.write_table(table, path, compression="uncompressed", stripe_size=64 << 20, row_index_stride=1000)
    rows = [orc.ORCFile(path).read_stripe(i).num_rows for i in range(orc.ORCFile(path).nstripes)]
    first = words[2500][:2]
    fewer = 0
    for pattern in (first + "%", first + "_%x", words[2500], words[2500] + "zz", "%" + first + "%", "_" + first[1:] + "%", "%", "\xff%", "c%c%",
                    words[0][:1] + "%", words[-1] + "%"):
        pred = P.like("s", pattern)
        mask = evaluate(pred, table)[0]
        _, (_, kept_f), (read_f, total_f) = check(path, table, rows, pred, 1000, mask=mask, prune=False)
        _, (_, kept_t), (read_t, total_t) = check(path, table, rows, pred, 1000, mask=mask, prune=True)
        assert kept_f == kept_t == int(mask.sum()) and read_f == total_f == total_t and read_t <= read_f, pattern
        fewer += read_t < read_f
        if pattern == first + "%":
            assert kept_t > 0 and read_t < read_f, (read_t, read_f)
        # under a NOT nothing is pruned, and nothing is lost
        nmask = evaluate(P.not_(pred), table)[0]
        _, _, (read_n, total_n) = check(path, table, rows, P.not_(pred), 1000, mask=nmask, prune=True)
        assert read_n == total_n
    assert fewer >= 4


def expect_refusal(builder, pred, code, word):
    r = builder.with_row_filter(pred, prune=False).build()
    with pytest.raises(capi.OrcGpuError) as e:
        next(r)
    assert e.value.code == code and word in str(e.value), (code, word, str(e.value))
    with pytest.raises(StopIteration):
        next(r)
    r.close()


def test_refusals_are_loud_and_name_the_column(tmpdir):
    path, table, rows = orc_file(tmpdir, "uncompressed")
    for prefetch in (0, 2):
        new = lambda: ArrowReaderBuilder.try_new(path, ctx()).with_prefetch(prefetch)
        expect_refusal(new(), P.like("bin", "a%"), MISMATCHED, "'bin'")
        expect_refusal(new(), P.like("v", "a%"), MISMATCHED, "'v'")
        expect_refusal(new().with_dictionary_columns(["s"]), P.like("s", "a%"), UNSUPPORTED, "'s'")
        expect_refusal(new().with_dictionary_columns(["s"]), P.like("s", "abc"), UNSUPPORTED, "'s'")
        expect_refusal(new(), P.like("s", "a%!", "!"), INVALID, "'s'")
        expect_refusal(new(), P.like("s", "a" * 1025), UNSUPPORTED, "'s'")
        expect_refusal(new(), P.like("s", "%".join("a" * 65)), UNSUPPORTED, "'s'")
        expect_refusal(new(), P.like("nope", "a%"), INVALID, "nope")
    nested = str(tmpdir / "nested.orc")
    orc.write_table(pa.table({"s": pa.array(["ab", "b", None]), "l": pa.array([[1], [], None], pa.list_(pa.int32()))}), nested)
    expect_refusal(ArrowReaderBuilder.try_new(nested, ctx()), P.like("s", "a%"), UNSUPPORTED, "'l'")
    # ... and the context is as usable as before: the same files filter
    got, _, _ = read(nested, P.like("s", "a%"), names=["s"])
    assert [b.column("s").to_pylist() for b in got] == [["ab"]]
    t, _ = like_mask(table, "a%", "\\")
    check(path, table, rows, P.like("s", "a%"), 1000, mask=t)
    got, _, _ = read(path, P.like("s", "a" * 1023 + "%"), names=["id", "s"])  # the longest pattern there is: 1024 with its wildcard
    assert got == []


def test_result_filter_on_a_hand_decoded_stripe_with_a_char_column():
    """orcgpu_result_filter straight after orcgpu_stripe_decode: a String column and a Char(8) column whose values carry their
    padding -- the pattern is matched against the whole exported value --, whole and under a row selection."""
    from orc_rust_amd import gen
    rng = np.random.default_rng(3)
    n, batch = 4097, 1000
    table = make_table()
    svals = table.column("s").to_pylist()
    present = np.array([v is not None for v in svals], np.uint8)
    sbytes = [v.encode() for v in svals if v is not None]
    chars = [random_text(rng, 9) for _ in range(n)]
    chars = [(c + " " * 8)[:8] for c in chars]  # Char(8): eight characters each, padded with spaces
    cbytes = [c.encode() for c in chars]
    ids = np.arange(n, dtype=np.int64)
    cols = [{"column_id": 1, "orc_type": 4, "encoding": 2}, {"column_id": 2, "orc_type": 7, "encoding": 2}, {"column_id": 3, "orc_type": 17, "encoding": 2}]
    streams = [(1, 1, gen.rle2(ids, signed=True)),
               (2, 0, gen.boolean(present)), (2, 1, b"".join(sbytes)), (2, 2, gen.rle2(np.array([len(x) for x in sbytes], dtype=np.int64), signed=False)),
               (3, 1, b"".join(cbytes)), (3, 2, gen.rle2(np.array([len(x) for x in cbytes], dtype=np.int64), signed=False))]
    c = ctx()
    cases = [(P.like("s", "%a%a%"), like_mask(table, "%a%a%", "\\")[0]),
             (P.not_like("s", "%c_abc"), like_mask(table, "%c_abc", "\\")[1]),
             (P.like("c8", "a%    "), np.array(LM.like_column(chars, "a%    "), bool)),
             (P.like("c8", "%b"), np.array(LM.like_column(chars, "%b"), bool)),  # (the padding is part of the value)
             (P.and_([P.like("c8", "_a______"), P.like("s", "%b%")]), np.array(LM.like_column(chars, "_a______"), bool) & like_mask(table, "%b%", "\\")[0])]
    assert all(0 < m.sum() < n for _, m in cases[:3]) and cases[4][1].sum() > 0
    for selection in (None, [(100, True), (2000, False), (1000, True), (997, False)]):
        for pred, mask in cases:
            staged = c.stage(n, streams, cols, batch_size=batch)
            res = c.decode([staged])[0]
            staged.free()
            in_rows = ids
            if selection is not None:
                res.select(selection)
                in_rows = np.concatenate([np.arange(s, s + k) for s, k in M.stripe_batches(M.normalise(selection), n, batch)])
            want = in_rows[mask[in_rows]]
            kept = c.result_filter(res, pred, ["id", "s", "c8"])
            assert kept == len(want) == res.rows and res.n_batches == (len(want) + batch - 1) // batch and res.status()[0] == 0
            res.fetch()
            if res.n_batches:
                exported = pa.Table.from_batches([res.export_batch(b) for b in range(res.n_batches)])
                assert exported.column(0).to_pylist() == want.tolist()
                assert exported.column(1).to_pylist() == [svals[k] for k in want] and exported.column(2).to_pylist() == [chars[k] for k in want]
            res.free()


def test_like_is_new():
    """What the parent commit answers: op 16 is an unknown op (ORCGPU_INVALID_ARGUMENT) and Predicate.like does not exist."""
    assert PR.LIKE == 16 and callable(P.like)
    from orc_rust_amd import gen
    ids = np.arange(3, dtype=np.int64)
    words = [b"ab", b"b", b"abc"]
    cols = [{"column_id": 1, "orc_type": 4, "encoding": 2}, {"column_id": 2, "orc_type": 7, "encoding": 2}]
    streams = [(1, 1, gen.rle2(ids, signed=True)), (2, 1, b"".join(words)), (2, 2, gen.rle2(np.array([len(x) for x in words], dtype=np.int64), signed=False))]
    c = ctx()
    staged = c.stage(3, streams, cols, batch_size=64)
    res = c.decode([staged])[0]
    staged.free()
    assert c.result_filter(res, P.like("s", "a%"), ["id", "s"]) == 2
    res.fetch()
    assert res.export_batch(0).column(1).to_pylist() == ["ab", "abc"]
    res.free()
