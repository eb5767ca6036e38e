"""Which leaf writes which mask plane: programs whose LIKE and IN leaves interleave, so that a leaf's plane number and its place in
its kernel's leaf list differ (filter_like_kernel / filter_in_kernel are launched over FilterPlan::like_leaves / in_leaves and
write the plane FilterInsn::i names; filter_eval_kernel reads it back).  Small files written here with pyarrow.orc, at row counts
around the 64-row mask word and the four-word workgroup, at batch sizes that do and do not divide a word, whole and under a row
selection; the rows to keep come from the Python models (filter_model, like_model, in_model) applied to the table."""
import decimal

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import filter_model as FM
import in_model as IM
import like_model as LM
import selection_model as M
from orc_rust_amd import capi, predicate as PR
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

ROWS = (1, 63, 64, 65, 257, 1025)  # 257 rows: five mask words, a second workgroup; 1025: several batches at either size
BATCH_SIZES = (64, 100)
D = decimal.Decimal
_CTX = None
_TABLES = {}
_FILES = {}


def ctx():
    global _CTX
    if _CTX is None:
        _CTX = capi.Context()
    return _CTX


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    capi.load()
    return tmp_path_factory.mktemp("row_filter_planes")


def word(k):
    """the string of row k: every leaf below matches some and misses some; values above 32 bytes take the wavefront's path"""
    r = k % 10
    if r == 0:
        return "a%db" % k                     # a_%b
    if r == 1:
        return "a" + "é" * 20 + "b"           # a_%b, 42 bytes
    if r == 2:
        return "w1%d" % k                     # w1%
    if r == 3:
        return "w1" + "x" * 40                # w1%, 42 bytes
    if r == 4:
        return ("mango", "kiwi", "fig" + "é" * 16)[k // 10 % 3]  # the IN list (its third key: 35 bytes)
    if r == 5:
        return "ab"                           # too short for a_%b
    if r == 6:
        return ""
    return "v%d" % (k * 7 % 13)


def make_table(n):
    """int64, string, Boolean and Decimal, about 10 % nulls each"""
    if n not in _TABLES:
        rng = np.random.default_rng(100 + n)

        def nulls(values):
            return [None if m else v for v, m in zip(values, rng.random(n) < 0.1)]

        _TABLES[n] = pa.table({
            "i": pa.array(nulls(rng.integers(0, 16, n).tolist()), pa.int64()),
            "s": pa.array(nulls([word(k) for k in range(n)]), pa.string()),
            "b": pa.array(nulls((rng.random(n) < 0.5).tolist()), pa.bool_()),
            "d": pa.array(nulls([D(int(x)).scaleb(-2) for x in rng.integers(-5000, 5000, n)]), pa.decimal128(10, 2)),
        })
    return _TABLES[n]


def orc_file(tmpdir, n):
    if n not in _FILES:
        path = str(tmpdir / ("planes_%d.orc" % n))
        orc.write_table(make_table(n), path, compression="uncompressed", stripe_size=64 << 20)
        assert orc.ORCFile(path).nstripes == 1
        _FILES[n] = path
    return _FILES[n]


# ---- the programs: leaf -> plane ----
def leaves():
    return [P.in_list("i", [V.Int64(x) for x in (1, 4, 7, 10, 13)]),               # plane 0
            P.like("s", "%"),                                                      # every valid row: no plane
            P.like("s", "a_%b"),                                                   # plane 1
            P.in_list("b", [V.Boolean(True), V.Boolean(None)]),                    # a Boolean list: no plane
            P.in_list("s", [V.Utf8("mango"), V.Utf8("kiwi"), V.Utf8("fig" + "é" * 16)]),  # plane 2
            P.like("s", "w1%")]                                                    # plane 3


def programs():
    """name -> predicate"""
    a = leaves()
    in_i, like_all, like_ab, in_b, in_s, like_w1 = a
    return {
        "or_of_all": P.or_(a),
        "or_reversed": P.or_(a[::-1]),  # the same leaves: planes 0 .. 3 are now LIKE, IN, LIKE, IN
        # (under the OR every valid string is kept by the `%` leaf: here each plane decides rows of its own)
        "each_plane_decides": P.or_([P.and_([in_i, like_ab]), P.and_([in_s, P.not_(like_w1)]), P.and_([P.not_(in_i), like_w1, in_b]), P.and_([P.not_(in_s), like_all, P.not_(in_b)])]),
        "only_like": P.and_([P.or_([like_ab, like_w1]), P.not_(P.like("s", "%1_"))]),
        "only_in": P.or_([P.and_([in_i, P.not_(in_s)]), P.in_list("d", [V.Decimal128((int(v.scaleb(2)), 2)) for v in (D("1.00"), D("-2.50"), D("7.77"))])]),
        "neither": P.or_([P.and_([P.gte("i", V.Int64(8)), P.lt("d", V.Decimal128((0, 2)))]), P.eq("s", V.Utf8("ab")), P.eq("b", V.Boolean(True))]),
    }


def like_leaf(pred, table):
    if pred.op == PR.LIKE:
        got = LM.like_column(table.column(pred.column).to_pylist(), pred.value.value, pred.escape)
        return np.array([g is True for g in got], bool), np.array([g is False for g in got], bool)
    return IM.FMT.evaluate(pred, table)


def keep_mask(pred, table):
    return IM.evaluate(pred, table, leaf=IM.in_leaf, other=like_leaf)[0]


def selection(n):
    """selected runs of 1, 63 and 65 rows (cut where the file ends); in the larger files they lie in different batches"""
    gaps = (1, 2) if n < 219 else (40, 50)
    return [(1, False), (gaps[0], True), (63, False), (gaps[1], True), (65, False)]


def test_the_programs_tell_a_plane_from_another():
    """On the CPU, from the models alone: what each program is here to show."""
    table = make_table(1025)
    for name in table.schema.names:
        assert 0.05 < table.column(name).null_count / 1025 < 0.15, name
    planes = [keep_mask(x, table) for k, x in enumerate(leaves()) if k in (0, 2, 4, 5)]
    for a in range(4):
        assert planes[a].any()
        for b in range(a):  # no two planes hold the same bits: a leaf that wrote another leaf's plane would show
            assert (planes[a] != planes[b]).any()
    for n in ROWS[1:]:  # every program keeps rows and drops rows (the OR of all leaves drops few: a row with a string is kept)
        t = make_table(n)
        for name, pred in programs().items():
            keep = keep_mask(pred, t)
            assert keep.any() and (not keep.all() or (name.startswith("or_") and n < 257)), (n, name)
    # swapping any two planes of "each_plane_decides" changes the rows it keeps
    lv = leaves()
    base = keep_mask(programs()["each_plane_decides"], table)
    for a, b in ((0, 2), (0, 4), (0, 5), (2, 4), (2, 5), (4, 5)):
        sw = list(lv)
        sw[a], sw[b] = lv[b], lv[a]
        in_i, like_all, like_ab, in_b, in_s, like_w1 = sw
        swapped = P.or_([P.and_([in_i, like_ab]), P.and_([in_s, P.not_(like_w1)]), P.and_([P.not_(in_i), like_w1, in_b]), P.and_([P.not_(in_s), like_all, P.not_(in_b)])])
        assert (keep_mask(swapped, table) != base).any(), (a, b)


def read(path, pred, batch_size, sel):
    b = ArrowReaderBuilder.try_new(path, ctx()).with_batch_size(batch_size)
    if sel is not None:
        b = b.with_row_selection(sel)
    r = b.with_row_filter(pred, prune=False).build()
    try:
        return list(r), r.filter_rows()
    finally:
        r.close()


def one(x):
    """a column as one Array"""
    return x if isinstance(x, pa.Array) else pa.concat_arrays(x.chunks) if x.num_chunks else pa.array([], x.type)


@pytest.mark.gpu
@pytest.mark.parametrize("batch_size", BATCH_SIZES)
@pytest.mark.parametrize("n", ROWS)
def test_every_leaf_writes_the_plane_the_evaluation_reads(tmpdir, n, batch_size):
    path, table = orc_file(tmpdir, n), make_table(n)
    for name, pred in programs().items():
        keep = keep_mask(pred, table)
        for sel in (None, selection(n)):
            idx = np.arange(n)
            if sel is not None:
                idx = np.concatenate([np.arange(s, s + m) for s, m in M.file_batches(sel, [n], batch_size)[0]]).astype(np.int64)
            kept = table.take(pa.array(idx[keep[idx]], pa.int64()))
            want = FM.rebatch(kept, [kept.num_rows], batch_size)
            got, (seen, n_kept) = read(path, pred, batch_size, sel)
            what = (n, batch_size, name, sel is not None)
            assert (seen, n_kept) == (len(idx), kept.num_rows), what
            assert [g.num_rows for g in got] == [w.num_rows for w in want], what
            for g, w in zip(got, want):
                g.validate(full=True)
                for col in w.schema.names:  # the kept rows, their validity and the null count the batch reports
                    a, b = one(g.column(col)), one(w.column(col))
                    assert a.cast(b.type).equals(b), what + (col,)
                    assert a.null_count == b.null_count and a.is_valid().equals(b.is_valid()), what + (col,)
