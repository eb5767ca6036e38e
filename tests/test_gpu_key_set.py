"""Key sets on the GPU: ArrowReaderBuilder.collect_keys builds a device-resident set, Predicate.in_set probes it.  The judge is the
numpy model of tests/key_set_model.py and, wherever a set fits an IN list (up to 65536 keys), the same read with
Predicate.in_list over the model's keys: the kept rows must be the same, row for row.  Files are written with pyarrow; a build or
probe side of more than 1024 rows under a tiny stripe_size is cut into stripes of 1024 rows."""
import datetime

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import key_set_model as M
from orc_rust_amd import KeySet, capi
from orc_rust_amd.aggregate import Agg
from orc_rust_amd.arrow_reader import ArrowReaderBuilder, concat_batches
from orc_rust_amd.key_set import SENTINEL
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

pytestmark = pytest.mark.gpu

BATCH = 1000
UNSUPPORTED, INVALID = 7, 101
_CTX = None
_FILES = {}


def ctx():
    global _CTX
    if _CTX is None:
        _CTX = capi.Context()
    return _CTX


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    capi.load()
    return tmp_path_factory.mktemp("key_set")


def write(tmpdir, name, table, stripes=1):
    """`table` as an ORC file of exactly `stripes` stripes (1024 rows each but the last)"""
    path = str(tmpdir / (name + ".orc"))
    orc.write_table(table, path, compression="uncompressed", row_index_stride=1000, stripe_size=(64 << 20) if stripes == 1 else 1024)
    assert table.num_rows == 0 or orc.ORCFile(path).nstripes == stripes, (name, orc.ORCFile(path).nstripes)
    return path


def nullable(values, valid, typ):
    return pa.array([int(v) if ok else None for v, ok in zip(values, valid)], typ)


class Side:
    """A build side: rows of (id, k, f) -- the key, nullable, and a column to filter by"""

    def __init__(self, tmpdir, name, keys, valid=None, f=None, stripes=1, typ=pa.int64()):
        n = len(keys)
        self.keys = np.asarray(keys, dtype=np.int64)
        self.valid = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
        self.f = np.arange(n, dtype=np.int64) % 10 if f is None else np.asarray(f, dtype=np.int64)
        table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "k": nullable(self.keys, self.valid, typ), "f": pa.array(self.f)})
        self.n, self.path = n, write(tmpdir, name, table, stripes)

    def builder(self, f_below=None, selection=None, prefetch=0):
        b = ArrowReaderBuilder.try_new(self.path, ctx()).with_batch_size(BATCH).with_prefetch(prefetch).with_projection(["id", "k", "f"])
        if selection is not None:
            b = b.with_row_selection(selection)
        if f_below is not None:
            b = b.with_row_filter(P.lt("f", V.Int64(f_below)), prune=False)
        return b

    def keep(self, f_below=None, selection=None):
        """(the rows the selection reads, the rows of them the filter keeps)"""
        seen = np.ones(self.n, bool)
        if selection is not None:
            seen[:] = False
            at = 0
            for count, skip in selection:
                if not skip:
                    seen[at:at + count] = True
                at += count
        kept = seen & (self.f < f_below) if f_below is not None else seen
        return seen, kept

    def model(self, f_below=None, selection=None):
        seen, kept = self.keep(f_below, selection)
        s, has_null = M.build(self.keys, kept, self.valid)
        return s, has_null, int(seen.sum())

    def collect(self, f_below=None, selection=None, max_keys=1 << 12, into=None, prefetch=0):
        return self.builder(f_below, selection, prefetch).collect_keys("k", max_keys=max_keys, into=into)


def check_set(ks, want):
    s, has_null, rows_seen = want
    assert (len(ks), ks.has_null, ks.rows_seen) == (len(s), has_null, rows_seen)


def probe_side(tmpdir):
    """The probe file: two stripes (1024 + 507 rows, neither a multiple of 64); Int, Long and Date keys, each with NULL rows, drawn
    so that about half of them hit the small build sides' keys (-40 .. 40); `c` to compare beside a set leaf"""
    if "probe" not in _FILES:
        n = 1531
        rng = np.random.default_rng(7)
        cols = {"id": np.arange(n, dtype=np.int64)}
        valid = {}
        for name in ("x32", "x64", "d"):
            cols[name] = rng.integers(-80, 81, n)
            valid[name] = rng.random(n) > 0.15
        cols["x64"][:4] = (M.INT64_MIN, M.INT64_MAX, SENTINEL, SENTINEL + 1)
        valid["x64"][:4] = True
        cols["c"] = rng.integers(0, 10, n)
        table = pa.table({"id": pa.array(cols["id"]), "x32": nullable(cols["x32"], valid["x32"], pa.int32()), "x64": nullable(cols["x64"], valid["x64"], pa.int64()),
                          "d": nullable(cols["d"], valid["d"], pa.int32()).cast(pa.date32()), "c": pa.array(cols["c"])})
        _FILES["probe"] = (write(tmpdir, "probe", table, stripes=2), cols, valid)
    return _FILES["probe"]


PROBE_COLS = ["id", "x32", "x64", "d", "c"]


def ids_of(reader):
    batches = list(reader)
    reader.close()
    return concat_batches(batches).column("id").to_pylist() if batches else []


def read_ids(path, pred, names=PROBE_COLS, prune=False, prefetch=0):
    b = ArrowReaderBuilder.try_new(path, ctx()).with_batch_size(BATCH).with_prefetch(prefetch).with_projection(list(names))
    return ids_of(b.with_row_filter(pred, prune=prune).build())


def literals(s, has_null):
    return [V.Int64(k) for k in sorted(s)] + ([V.Int64(None)] if has_null else [])


def check_probe(tmpdir, ks, want, columns=("x64",), negate=False):
    """in_set == in_list over the model's keys == the numpy model, row for row, on the probe file"""
    path, cols, valid = probe_side(tmpdir)
    s, has_null, _ = want
    for col in columns:
        a = M.in_set(cols[col], valid[col], s, has_null)
        p_set, p_list = P.in_set(col, ks), P.in_list(col, literals(s, has_null))
        if negate:
            a, p_set, p_list = M.not_(a), P.not_(p_set), P.not_(p_list)
        model = M.kept(a).tolist()
        got = read_ids(path, p_set)
        assert got == model, (col, negate, len(got), len(model))
        assert read_ids(path, p_list) == model, (col, negate)


# ---- build sides where the build can go wrong ----
@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097))
def test_build_sides_of_every_size(tmpdir, n):
    rng = np.random.default_rng(n)
    side = Side(tmpdir, "size%d" % n, rng.integers(-40, 41, n), rng.random(n) > 0.1 if n > 1 else None, stripes=(n + 1023) // 1024)
    with side.collect() as ks:
        check_set(ks, side.model())
        check_probe(tmpdir, ks, side.model(), columns=("x32", "x64", "d"))


def test_all_rows_one_key_all_rows_null_and_no_row_kept(tmpdir):
    one = Side(tmpdir, "one_key", np.full(300, 17))
    with one.collect() as ks:
        check_set(ks, ({17}, False, 300))
        check_probe(tmpdir, ks, one.model())
    nulls = Side(tmpdir, "all_null", np.zeros(300), valid=np.zeros(300, bool))
    with nulls.collect() as ks:
        check_set(ks, (set(), True, 300))
        check_probe(tmpdir, ks, nulls.model())                   # UNKNOWN everywhere: nothing kept ...
        check_probe(tmpdir, ks, nulls.model(), negate=True)      # ... under a NOT too
    with one.collect(f_below=-1) as ks:                          # the filter keeps no row: the empty set, FALSE everywhere
        check_set(ks, (set(), False, 300))
        check_probe(tmpdir, ks, (set(), False, 300))
        check_probe(tmpdir, ks, (set(), False, 300), negate=True)    # NOT FALSE: every row, the NULL rows included


def test_a_key_equal_to_the_sentinel_alone_and_among_others(tmpdir):
    alone = Side(tmpdir, "sentinel_alone", [SENTINEL, SENTINEL, SENTINEL])
    with alone.collect() as ks:
        check_set(ks, ({SENTINEL}, False, 3))
        check_probe(tmpdir, ks, alone.model())
    rng = np.random.default_rng(3)
    keys = rng.integers(-40, 41, 500)
    keys[[0, 77, 499]] = SENTINEL
    keys[[1, 2]] = (M.INT64_MIN, M.INT64_MAX)
    valid = rng.random(500) > 0.1
    valid[[0, 1, 2]] = True
    among = Side(tmpdir, "sentinel_among", keys, valid)
    with among.collect() as ks:
        assert SENTINEL in among.model()[0]
        check_set(ks, among.model())
        check_probe(tmpdir, ks, among.model())
        check_probe(tmpdir, ks, among.model(), negate=True)


def test_a_build_under_a_row_filter_a_row_selection_and_both(tmpdir):
    rng = np.random.default_rng(11)
    side = Side(tmpdir, "filtered", rng.integers(-40, 41, 2500), rng.random(2500) > 0.05, f=rng.integers(0, 10, 2500), stripes=3)
    sel = [(100, True), (900, False), (700, True), (450, False), (350, True)]
    for kw in ({"f_below": 3}, {"selection": sel}, {"f_below": 2, "selection": sel}):
        with side.collect(**kw) as ks:
            check_set(ks, side.model(**kw))
            check_probe(tmpdir, ks, side.model(**kw))


def test_three_stripes_and_two_readers_into_one_set(tmpdir):
    rng = np.random.default_rng(12)
    a = Side(tmpdir, "three_a", rng.integers(-40, 0, 2500), rng.random(2500) > 0.02, stripes=3)
    b = Side(tmpdir, "three_b", rng.integers(-5, 41, 700))
    for prefetch in (0, 2):
        with a.collect(prefetch=prefetch) as ks:
            check_set(ks, a.model())
    with KeySet(ctx(), 1 << 10) as ks:
        assert a.collect(into=ks) is ks and not ks.sealed
        b.collect(f_below=5, into=ks)
        sa, na, ra = a.model()
        sb, nb, rb = b.model(f_below=5)
        with pytest.raises(ValueError):      # not sealed yet
            len(ks)
        ks.seal()
        check_set(ks, (sa | sb, na or nb, ra + rb))
        check_probe(tmpdir, ks, (sa | sb, na or nb, ra + rb))
        with pytest.raises(ValueError):      # sealed: no further collect
            b.collect(into=ks)


# ---- collisions ----
@pytest.mark.parametrize("bits", ("1", "4"))
def test_a_masked_hash_gives_long_chains_and_the_same_membership(tmpdir, monkeypatch, bits):
    keys = np.arange(300, dtype=np.int64) * 3 - 450       # 300 distinct keys, -450 .. 447
    side = Side(tmpdir, "chain", keys)
    monkeypatch.setenv("ORCGPU_KEY_SET_HASH_BITS", bits)
    # 1024 slots, every chain starts in the last 2 / 16 of them: the run of 300 occupied slots wraps round the table's end
    with side.collect(max_keys=300) as ks:
        monkeypatch.delenv("ORCGPU_KEY_SET_HASH_BITS")      # (the mask is the set's from its creation on)
        check_set(ks, side.model())
        check_probe(tmpdir, ks, side.model(), columns=("x32", "x64"))


def test_exactly_the_limit_fits_and_one_more_is_refused(tmpdir):
    fits = Side(tmpdir, "fits32", np.repeat(np.arange(32), 3))
    with fits.collect(max_keys=32) as ks:
        check_set(ks, fits.model())
        check_probe(tmpdir, ks, fits.model())
    over = Side(tmpdir, "over33", np.repeat(np.arange(33), 3))
    with pytest.raises(capi.OrcGpuError) as e:
        over.collect(max_keys=32)
    assert e.value.code == UNSUPPORTED and "32" in str(e.value) and "key set" in str(e.value)
    with KeySet(ctx(), 32) as ks:
        over.collect(into=ks)
        with pytest.raises(capi.OrcGpuError) as e:
            ks.seal()
        assert e.value.code == UNSUPPORTED and "32" in str(e.value)
        path, _, _ = probe_side(tmpdir)
        with pytest.raises(capi.OrcGpuError) as e:
            read_ids(path, P.in_set("x64", ks))
        assert e.value.code == INVALID and "unusable" in str(e.value) and "'x64'" in str(e.value)


# ---- both probe paths: a table of up to 32 KiB is staged in LDS, a larger one is probed in global memory ----
@pytest.mark.parametrize("n_keys", (1000, 5000))
def test_the_lds_path_and_the_global_memory_path(tmpdir, n_keys):
    rng = np.random.default_rng(n_keys)
    keys = rng.choice(np.arange(-n_keys, n_keys), n_keys, replace=False)
    keys[:40] = np.arange(-20, 20)                          # (some the probe side holds)
    side = Side(tmpdir, "path%d" % n_keys, keys, stripes=(n_keys + 1023) // 1024)
    with side.collect(max_keys=n_keys) as ks:               # 2048 slots: 16.6 KiB; 16384 slots: 130 KiB
        assert len(ks) == len(set(keys.tolist()))
        check_probe(tmpdir, ks, side.model(), columns=("x32", "x64", "d"))


def test_past_the_in_list_70000_keys_probed_by_200000_rows(tmpdir):
    rng = np.random.default_rng(70)
    keys = rng.choice(np.arange(-(1 << 20), 1 << 20), 70_000, replace=False)
    side = Side(tmpdir, "big_build", keys)
    x = rng.integers(-(1 << 20), 1 << 20, 200_000)
    valid = rng.random(200_000) > 0.05
    path = write(tmpdir, "big_probe", pa.table({"id": pa.array(np.arange(200_000, dtype=np.int64)), "x": nullable(x, valid, pa.int64())}))
    with side.collect(max_keys=1 << 17, prefetch=2) as ks:
        check_set(ks, (set(keys.tolist()), False, 70_000))
        model = M.kept(M.in_set(x, valid, set(keys.tolist()), False)).tolist()
        assert 5000 < len(model) < 10000
        assert read_ids(path, P.in_set("x", ks), names=["id", "x"], prefetch=2) == model


# ---- logic ----
def test_not_and_or_two_sets_and_pruning(tmpdir):
    path, cols, valid = probe_side(tmpdir)
    rng = np.random.default_rng(13)
    a = Side(tmpdir, "logic_a", rng.integers(-40, 10, 400))
    b = Side(tmpdir, "logic_b", rng.integers(-10, 41, 400), rng.random(400) > 0.1)
    with a.collect() as ka, b.collect() as kb:
        (sa, na, _), (sb, nb, _) = a.model(), b.model()
        assert not na and nb
        ma, mb = M.in_set(cols["x64"], valid["x64"], sa, na), M.in_set(cols["x32"], valid["x32"], sb, nb)
        mc = M.compare(cols["c"], None, ">=", 5)
        ml = M.in_set(cols["d"], valid["d"], {-3, 0, 7, 11}, False)
        pc, pl = P.gte("c", V.Int64(5)), P.in_list("d", [V.Int32(v) for v in (-3, 0, 7, 11)])
        for pred, model in ((P.not_in_set("x64", ka), M.not_(ma)),                                     # without has_null: the non-matches
                            (P.not_in_set("x32", kb), M.not_(mb)),                                     # with: nothing
                            (P.and_([P.in_set("x64", ka), pc]), M.and_(ma, mc)),
                            (P.or_([P.in_set("x64", ka), pc, pl]), M.or_(M.or_(ma, mc), ml)),
                            (P.and_([P.or_([P.in_set("x64", ka), P.in_set("x32", kb)]), P.not_(pl)]), M.and_(M.or_(ma, mb), M.not_(ml))),
                            (P.or_([P.not_in_set("x64", ka), P.and_([P.in_set("x32", kb), pc])]), M.or_(M.not_(ma), M.and_(mb, mc)))):
            want = M.kept(model).tolist()
            assert read_ids(path, pred, prune=False) == want, pred
            assert read_ids(path, pred, prune=True) == want, pred
        assert M.kept(M.not_(mb)).tolist() == []


def test_as_an_aggregates_condition_and_as_the_top_ks_filter(tmpdir):
    path, cols, valid = probe_side(tmpdir)
    side = Side(tmpdir, "agg_build", np.random.default_rng(14).integers(-40, 41, 300))
    s, has_null, _ = side.model()

    def builder():
        return ArrowReaderBuilder.try_new(path, ctx()).with_batch_size(BATCH).with_prefetch(0).with_projection(PROBE_COLS)
    with side.collect() as ks:
        m = M.in_set(cols["x64"], valid["x64"], s, has_null)
        specs = lambda p: [Agg.count_rows().where(p), Agg.sum("c").where(p), Agg.count_rows()]      # noqa: E731
        got = builder().aggregate(specs(P.in_set("x64", ks)))
        assert got == builder().aggregate(specs(P.in_list("x64", literals(s, has_null))))
        assert got == [int(m[0].sum()), int(cols["c"][m[0]].sum()), 1531]
        top = lambda p: builder().with_row_filter(p, prune=False).top_k([("c", "desc"), "id"], 50).column("id").to_pylist()   # noqa: E731
        got = top(P.in_set("x64", ks))
        assert got == top(P.in_list("x64", literals(s, has_null)))
        order = sorted(M.kept(m).tolist(), key=lambda i: (-int(cols["c"][i]), i))[:50]
        assert got == order


# ---- refusals, with status and message ----
def typed_file(tmpdir):
    n = 100
    table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "ts": pa.array([datetime.datetime(2020, 1, 1) + datetime.timedelta(seconds=i) for i in range(n)], pa.timestamp("ns")),
                      "dec": pa.array([__import__("decimal").Decimal(i) for i in range(n)], pa.decimal128(10, 2)), "s": pa.array(["s%d" % (i % 7) for i in range(n)]),
                      "f": pa.array(np.arange(n, dtype=np.float64)), "b": pa.array([i % 2 == 0 for i in range(n)])})
    return write(tmpdir, "typed", table)


def refused(fn, code, *words):
    with pytest.raises(capi.OrcGpuError) as e:
        fn()
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_refusals_on_either_side(tmpdir):
    path = typed_file(tmpdir)
    names = ["id", "ts", "dec", "s", "f", "b"]

    def builder(dictionary=None):
        b = ArrowReaderBuilder.try_new(path, ctx()).with_batch_size(BATCH).with_prefetch(0).with_projection(names)
        return b.with_dictionary_columns(dictionary) if dictionary else b
    with Side(tmpdir, "ref_build", np.arange(10)).collect() as ks:
        for col, word in (("ts", "Timestamp"), ("dec", "Decimal"), ("s", "String"), ("f", "Float"), ("b", "Boolean")):
            refused(lambda: builder().collect_keys(col, max_keys=64), UNSUPPORTED, "'%s'" % col, word, "key set")                         # the build side
            refused(lambda: ids_of(builder().with_row_filter(P.in_set(col, ks), prune=False).build()), UNSUPPORTED, "'%s'" % col, word)   # the probe side
        refused(lambda: builder(["s"]).collect_keys("s"), UNSUPPORTED, "'s'")
        refused(lambda: ids_of(builder(["s"]).with_row_filter(P.in_set("s", ks), prune=False).build()), UNSUPPORTED, "'s'")
        refused(lambda: builder().collect_keys("nope"), INVALID, "'nope'", "not a projected root column")
        refused(lambda: ArrowReaderBuilder.try_new(path, ctx()).with_projection(["ts"]).collect_keys("id"), INVALID, "'id'")          # unprojected
        refused(lambda: ids_of(builder().with_row_filter(P.in_set("nope", ks), prune=False).build()), INVALID, "'nope'")
    with KeySet(ctx(), 64) as open_set:                                                                                     # an unsealed set
        refused(lambda: ids_of(builder().with_row_filter(P.in_set("id", open_set), prune=False).build()), INVALID, "'id'", "not sealed")
    other = capi.Context()                                                                                                   # a set of another context
    try:
        with Side(tmpdir, "ref_build", np.arange(10)).collect() as ks:
            b = ArrowReaderBuilder.try_new(path, other).with_batch_size(BATCH).with_prefetch(0).with_projection(names)
            refused(lambda: ids_of(b.with_row_filter(P.in_set("id", ks), prune=False).build()), INVALID, "'id'", "not a set of this context")
            foreign = KeySet(other, 64)
            refused(lambda: builder().collect_keys("id", into=foreign), INVALID, "another context")
            foreign.close()
    finally:
        other.close()


# ---- lifetime, and what stays untouched ----
def test_closing_a_set_does_not_disturb_a_reader_that_filters_by_it(tmpdir):
    path, cols, valid = probe_side(tmpdir)
    side = Side(tmpdir, "life", np.arange(-40, 41, 2))
    ks = side.collect()
    s, has_null, _ = side.model()
    r = ArrowReaderBuilder.try_new(path, ctx()).with_batch_size(100).with_prefetch(0).with_projection(PROBE_COLS).with_row_filter(P.in_set("x64", ks), prune=False).build()
    first = next(r)                          # 100 of the kept rows; the rest of the file is still to be handed out
    ks.close()
    junk = [KeySet(ctx(), 1 << 10) for _ in range(4)]       # (allocations that would take the freed memory, were it freed)
    rest = list(r)
    r.close()
    for k in junk:
        k.close()
    got = concat_batches([first] + rest).column("id").to_pylist()
    assert got == M.kept(M.in_set(cols["x64"], valid["x64"], s, has_null)).tolist()
    assert max(got) >= 1024                  # rows of the second stripe among them


def test_a_collecting_reader_copies_nothing_back_and_hands_out_no_batch(tmpdir):
    rng = np.random.default_rng(15)
    side = Side(tmpdir, "d2h", rng.integers(-40, 41, 2500), stripes=3)
    for prefetch in (0, 2):
        with KeySet(ctx(), 1 << 10) as ks:
            r = side.builder(f_below=5, prefetch=prefetch).build()
            assert r.collect_keys("k", ks) is ks
            assert r.d2h_bytes() == 0 and r.filter_rows()[0] == 2500
            refused(lambda: next(r), INVALID, "hands out no batches")
            r.close()
            ks.seal()
            check_set(ks, side.model(f_below=5))


def test_an_in_list_program_keeps_the_rows_it_kept_before(tmpdir):
    # (the library counts no kernel launches: that a program without a set leaf launches what it launched before is read off
    # filter_run_eval, whose launches depend on the plan's leaf lists alone; here: the same rows, beside a live set and without one)
    path, cols, valid = probe_side(tmpdir)
    keys = set(range(-30, 31, 3))
    want = M.kept(M.in_set(cols["x32"], valid["x32"], keys, False)).tolist()
    pred = P.in_list("x32", [V.Int32(k) for k in sorted(keys)])
    assert read_ids(path, pred) == want
    with Side(tmpdir, "beside", np.arange(5)).collect():
        assert read_ids(path, pred) == want
