"""SQL IN in the row filter on the GPU (ORCGPU_PRED_IN: filter_in_kernel in device/filter_kernels.hip, the hash sets built by
orcgpu_in.inc) against the model of tests/in_model.py -- x IN (v1 .. vk) is OR(x = v1, ..., x = vk) --: files written here with
pyarrow.orc, filtered per stripe by the model and rebatched: the reader must hand out exactly those batches, and for short lists
exactly the batches of its own read of the OR of the EQ leaves."""
import datetime
import decimal
import os

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

N = 4097
BATCH_SIZES = (64, 1000)
COMPRESSIONS = ("uncompressed", "zlib")
MISMATCHED, UNSUPPORTED, INVALID = 6, 7, 101
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
NAN, INF = float("nan"), float("inf")
D = decimal.Decimal
DAY0 = datetime.date(1970, 1, 1)
TS0 = 1577836800 * 10 ** 9  # 2020-01-01T00:00:00 in nanoseconds
_CTX = None
_FILES = {}
_TABLE = None
_CASES = None
_MASKS = {}


def ctx():
    global _CTX
    if _CTX is None:
        _CTX = capi.Context()
    return _CTX


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    capi.load()  # (sets TZDIR where the system has no tz database: pyarrow's ORC writer needs one for the Timestamp column)
    return tmp_path_factory.mktemp("row_filter_in")


def word(k, prefix=""):
    """the string of row k: lengths 0, 1, 31, 32, 33 and 90 bytes in turn, multi-byte text among them, then short ones"""
    tag, r = "%s%05d" % (prefix, k), k % 8
    if r == 0:
        return "" if not prefix else prefix
    if r == 1:
        return (prefix or "abcdefghijklmnopqrstuvwxyz")[k // 8 % (1 if prefix else 26)]
    if r == 2:
        return tag + "é" * 13                  # 31 bytes
    if r == 3:
        return tag + "x" + "é" * 13            # 32
    if r == 4:
        return tag + "é" * 14                  # 33
    if r == 5:
        return tag + "x" + "é" * 42            # 90
    return "w%d" % (k // 8) if not prefix else "%sw%d" % (prefix, k // 8)


def make_table():
    """Every column holds EVEN numbers (and its planted specials), so that odd ones lie outside it; about 20 % nulls per column."""
    global _TABLE
    if _TABLE is None:
        rng = np.random.default_rng(23)

        def nulls(values):
            return [None if m else v for v, m in zip(values, rng.random(N) < 0.2)]

        i64 = [int(x) * 2 for x in rng.integers(-2 ** 61, 2 ** 61, N)]
        for k, v in enumerate((I64_MIN, -1, 0, I64_MAX)):
            i64[k::400] = [v] * len(i64[k::400])
        fl = [NAN, 0.0, -0.0, INF, -INF]
        f64 = [fl[k % 16] if k % 16 < len(fl) else float(x) / 10 * 2 for k, x in enumerate(rng.integers(-500, 500, N))]
        f32 = [fl[k % 16] if k % 16 < len(fl) else float(np.float32(float(x) / 10 * 2)) for k, x in enumerate(rng.integers(-500, 500, N))]
        s = [word(k) for k in range(N)]
        _TABLE = pa.table({
            "id": pa.array(np.arange(N, dtype=np.int64)),
            "i8": pa.array(nulls((rng.integers(-64, 64, N) * 2).tolist()), pa.int8()),
            "i16": pa.array(nulls((rng.integers(-15000, 15000, N) * 2).tolist()), pa.int16()),
            "i32": pa.array(nulls((rng.integers(-10 ** 9, 10 ** 9, N) * 2).tolist()), pa.int32()),
            "i64": pa.array(nulls(i64), pa.int64()),
            "date": pa.array(nulls([DAY0 + datetime.timedelta(days=int(x) * 2) for x in rng.integers(-4000, 4000, N)]), pa.date32()),
            "f32": pa.array(nulls(f32), pa.float32()),
            "f64": pa.array(nulls(f64), pa.float64()),
            "b": pa.array(nulls((rng.random(N) < 0.5).tolist()), pa.bool_()),
            "s": pa.array(nulls(s), pa.string()),
            "bin": pa.array(nulls([x.encode()[::-1] for x in s]), pa.binary()),
            "dec": pa.array(nulls([D(int(x) * 2).scaleb(-2) for x in rng.integers(-10 ** 6, 10 ** 6, N)]), pa.decimal128(10, 2)),
            "dec38": pa.array(nulls([D(int(x) * 2 * 10 ** 16) for x in rng.integers(-10 ** 18, 10 ** 18, N)]), pa.decimal128(38, 0)),
            "ts": pa.array(nulls([TS0 + int(x) * 2000 for x in rng.integers(0, 10 ** 9, N)]), pa.timestamp("ns")),
            "allnull": pa.array([None] * N, pa.int32()),
        })
    return _TABLE


def orc_file(tmpdir, compression):
    """(path, the file's rows as the reader itself hands them out unfiltered, rows per stripe)"""
    if compression not in _FILES:
        path = str(tmpdir / ("in_%s.orc" % compression))
        table = make_table()
        orc.write_table(table, path, compression=compression, stripe_size=1024, row_index_stride=1000, batch_size=1500 if compression == "uncompressed" else 300)
        f = orc.ORCFile(path)
        rows = [f.read_stripe(i).num_rows for i in range(f.nstripes)]
        assert f.nstripes >= 2, rows
        plain = pa.Table.from_batches(read(path, None, batch_size=8192)[0])
        assert plain.num_rows == N
        for name in table.schema.names:  # the unfiltered read is the table the model judges (Timestamp: the same instants)
            a, b = plain.column(name), table.column(name)
            if name == "ts":
                a, b = a.cast(pa.timestamp("ns")).cast(pa.int64()), b.cast(pa.int64())
            assert same_column(a, b), name
        _FILES[compression] = (path, plain, rows)
    return _FILES[compression]


# ---- the lists ----
def own(name):
    """the column's distinct values, sorted"""
    col = make_table().column(name)
    vals = {v for v in (col.cast(pa.int64()) if name == "ts" else col).to_pylist() if v is not None and v == v}
    return sorted(vals)


def lit(name, v):
    """the PredicateValue of the kind column `name` takes"""
    if name in ("i8", "i16", "i32", "i64", "allnull", "id"):
        return {"i8": V.Int8, "i16": V.Int16, "i32": V.Int32}.get(name, V.Int64)(v)
    if name == "date":
        return V.Int32(None if v is None else (v - DAY0).days if isinstance(v, datetime.date) else v)
    if name in ("f32", "f64"):
        return (V.Float32 if name == "f32" else V.Float64)(v)
    if name == "b":
        return V.Boolean(v)
    if name in ("dec", "dec38"):
        return V.Decimal128(v)
    if name == "ts":
        return V.TimestampNs(v)
    return V.Utf8(v)


def outside(name, k):
    """a value of the column's kind that no row holds (the columns hold even numbers), the k-th of them"""
    if name in ("i8",):
        return -127 + 2 * (k % 127)
    if name in ("i16", "i32", "i64", "date"):
        return 2 * k + 1 + (10 ** 6 if name in ("i32", "i64") else 0)
    if name in ("f32", "f64"):
        return k + 0.5
    if name in ("dec", "dec38"):
        return D(2 * k + 1).scaleb(-2) if name == "dec" else D(2 * k + 1)
    if name == "ts":
        return TS0 + (2 * k + 1) * 1000
    w = word(k, "Z")
    return w.encode()[::-1] if name == "bin" else w


def mixed(name, size, seed=1):
    """`size` literals: half drawn from every other one of the column's own values (so that rows are kept AND dropped), with
    repeats where the column has too few, half from outside; shuffled"""
    rng = np.random.default_rng(seed + size)
    pool = own(name)[::2]
    n_own = size // 2
    picks = rng.permutation(len(pool))[:n_own] if n_own <= len(pool) else rng.integers(0, len(pool), n_own)
    vals = [pool[int(k)] for k in picks] + [outside(name, k) for k in range(size - n_own)]
    return [lit(name, vals[int(k)]) for k in rng.permutation(len(vals))]


SIZED = ("i8", "i16", "i32", "i64", "date", "f32", "f64", "s", "bin", "dec", "dec38", "ts")
# the named degenerate lists: they keep no row (NOT IN () keeps every row)
DEGENERATE = ("empty", "only_nulls", "only_nan", "only_off_scale", "not_in_with_null", "not_only_nulls", "allnull")
KEEP_ALL = ("not_empty",)


def cases():
    """name -> predicate"""
    global _CASES
    if _CASES is not None:
        return _CASES
    c = {}
    for name in SIZED:
        for size in (1, 2, 3, 16):
            c["%s_%d" % (name, size)] = P.in_list(name, mixed(name, size) if size > 1 else [lit(name, own(name)[len(own(name)) // 2])])
    for name in ("i64", "s"):
        c["%s_5000" % name] = P.in_list(name, mixed(name, 5000))  # a table above 32 KiB: probed in global memory
    c["i64_65536"] = P.in_list("i64", mixed("i64", 65536))
    c["bin_600"] = P.in_list("bin", mixed("bin", 600))  # a string table that is still staged in LDS
    c["empty"] = P.in_list("i32", [])
    c["not_empty"] = P.not_in("i32", [])
    c["only_nulls"] = P.in_list("i64", [V.Int64(None), V.Int8(None)])
    c["not_only_nulls"] = P.not_in("s", [V.Utf8(None)])
    c["with_null"] = P.in_list("i16", mixed("i16", 6) + [V.Int16(None)])
    c["not_in_with_null"] = P.not_in("i16", mixed("i16", 6) + [V.Int16(None)])
    c["one_with_null"] = P.in_list("s", [V.Utf8(own("s")[7]), V.Utf8(None)])
    c["duplicates"] = P.in_list("i32", mixed("i32", 8) * 3)
    c["mixed_kinds"] = P.in_list("i8", [V.Int64(own("i8")[3]), V.Int16(own("i8")[9]), V.Int8(own("i8")[20]), V.Int32(300), V.Int64(I64_MIN)])
    c["i64_edges"] = P.in_list("i64", [V.Int64(I64_MIN), V.Int64(-1), V.Int64(0), V.Int64(I64_MAX), V.Int64(1)])
    c["not_i64_edges"] = P.not_in("i64", [V.Int64(I64_MIN), V.Int64(-1), V.Int64(0), V.Int64(I64_MAX)])
    c["not_in_16"] = P.not_in("date", mixed("date", 16))
    c["not_in_strings"] = P.not_in("s", mixed("s", 16) + [V.Utf8("")])
    # the float corners: a NaN literal equals no row, the two zeros are one key, a Float32 literal is rounded through float
    c["only_nan"] = P.in_list("f64", [V.Float64(NAN), V.Float32(NAN)])
    c["nan_and_more"] = P.in_list("f64", [V.Float64(NAN), V.Float64(INF), V.Float64(own("f64")[5])])
    c["minus_zero"] = P.in_list("f64", [V.Float64(-0.0), V.Float64(-INF)])
    c["zero_on_f32"] = P.in_list("f32", [V.Float32(0.0), V.Float64(INF)])
    f32_own = [v for v in own("f32") if 1 < abs(v) < 1000][:3]  # (the doubles that the column's floats are, exactly)
    c["float32_rounded"] = P.in_list("f32", [V.Float32(round(v, 1)) for v in f32_own] + [V.Float32(0.3)])
    c["float64_on_f32_misses"] = P.in_list("f32", [V.Float64(0.2), V.Float64(-0.2), V.Float64(f32_own[0])])
    c["not_in_floats"] = P.not_in("f32", [V.Float32(NAN), V.Float32(0.0), V.Float32(INF)])
    c["bool_both"] = P.and_([P.in_list("b", [V.Boolean(True), V.Boolean(False)]), P.lt("id", V.Int64(3000))])
    c["not_bool_both"] = P.or_([P.not_in("b", [V.Boolean(True), V.Boolean(False)]), P.in_list("i8", [V.Int8(0), V.Int8(2)])])
    c["bool_with_null"] = P.in_list("b", [V.Boolean(False), V.Boolean(None)])
    c["not_bool_with_null"] = P.or_([P.not_in("b", [V.Boolean(False), V.Boolean(None)]), P.in_list("i8", [V.Int8(0), V.Int8(2)])])
    # Decimal: literals at another scale that match, and one that equals nothing
    d = own("dec")
    c["dec_other_scales"] = P.in_list("dec", [V.Decimal128((int(d[5].scaleb(2)) * 10, 3)), V.Decimal128((int(d[40].scaleb(2)) * 10 ** 10, 12)), V.Decimal128((12345, 3))])
    whole = [v for v in d if v == v.to_integral_value()][:2]
    c["dec_lower_scale"] = P.in_list("dec", [V.Decimal128((int(v), 0)) for v in whole] + [V.Decimal128((7, 1))])
    c["only_off_scale"] = P.in_list("dec", [V.Decimal128((12345, 3)), V.Decimal128((1, 38))])
    c["not_off_scale"] = P.and_([P.not_in("dec", [V.Decimal128((12345, 3))]), P.lt("id", V.Int64(900))])
    c["dec38_beyond"] = P.in_list("dec38", [V.Decimal128((10 ** 38 - 1, 0)), V.Decimal128(own("dec38")[3]), V.Decimal128((int(own("dec38")[9]) * 1000, 3))])
    # Timestamp (nanoseconds in the file): every literal lands on a value; a datetime literal among them
    t = own("ts")
    c["ts_instants"] = P.in_list("ts", [V.TimestampNs(t[3]), V.TimestampNs(t[100]), V.TimestampNs(t[100] + 1), V.TimestampNs(None)])
    # trees: beside comparisons and a LIKE leaf, two IN leaves on different columns in one program
    a, b = P.in_list("i16", mixed("i16", 16)), P.in_list("s", mixed("s", 16) + [V.Utf8("")])
    c["and_cmp"] = P.and_([a, P.gt("i32", V.Int32(0))])
    c["or_like"] = P.or_([b, P.like("s", "w1%")])
    c["two_leaves"] = P.and_([P.not_(a), P.or_([b, P.is_null("i16")])])
    c["two_tables_like"] = P.or_([P.and_([P.in_list("i64", mixed("i64", 5000)), P.in_list("bin", mixed("bin", 16))]), P.like("s", "%" + "é" * 14),
                                  P.in_list("dec", mixed("dec", 3))])
    c["not_tree"] = P.not_(P.or_([a, b, P.in_list("ts", mixed("ts", 16)), P.lt("i32", V.Int32(-10 ** 9))]))
    c["allnull"] = P.in_list("allnull", [V.Int32(1), V.Int32(2)])
    c["between"] = P.and_([P.between("i16", V.Int16(-100), V.Int16(100)), P.in_list("b", [V.Boolean(True)])])
    _CASES = c
    return c


def columns_of(pred):
    return ({pred.column} if pred.column is not None else set()).union(*[columns_of(k) for k in pred.children])


def n_literals(pred):
    return len(pred.children) if pred.op == PR.IN else sum(n_literals(k) for k in pred.children)


def like_leaf(pred, table):
    if pred.op == PR.LIKE:
        got = LM.like_column(table.column(pred.column).to_pylist(), pred.value.value, pred.escape)
        return np.array([g is True for g in got], bool), np.array([g is False for g in got], bool)
    return IM.FMT.evaluate(pred, table)


def mask(name):
    """(TRUE rows, FALSE rows) of a case over the whole table, by the model, computed once.  Lists of at most 16 literals by the
    definition (the OR of the EQ leaves); longer ones through the set, which tests/test_in_model.py holds to the definition."""
    if name not in _MASKS:
        pred = cases()[name]
        leaf = IM.in_leaf if n_literals(pred) <= 16 else IM.in_leaf_by_set
        _MASKS[name] = IM.evaluate(pred, make_table(), leaf=leaf, other=like_leaf)
    return _MASKS[name]


def test_the_inputs_tell_a_probe_that_answers_all_or_none():
    """On the CPU, from the model alone: apart from the named degenerate lists every case keeps a row and drops a valid row, so
    neither "every row" nor "no row" can pass the comparisons below; and the table holds what the issue asks for."""
    table = make_table()
    for name in table.schema.names[1:-1]:
        assert 0.15 < table.column(name).null_count / N < 0.25, name
    assert table.column("allnull").null_count == N
    assert {I64_MIN, -1, 0, I64_MAX} <= set(own("i64"))
    for name in ("f32", "f64"):
        vals = [v for v in table.column(name).to_pylist() if v is not None]
        assert any(v != v for v in vals) and INF in vals and -INF in vals and any(str(v) == "-0.0" for v in vals) and any(str(v) == "0.0" for v in vals)
    lens = {len(v.encode()) for v in own("s")}
    assert {0, 1, 31, 32, 33, 90} <= lens and any(len(v) != len(v.encode()) for v in own("s"))
    for name, pred in cases().items():
        t, f = mask(name)
        assert not (t & f).any()
        valid = np.ones(N, bool)  # rows without a null in the columns the case names
        for col in columns_of(pred):
            valid &= np.array(table.column(col).is_valid().to_pylist(), bool)
        if name in DEGENERATE:
            assert t.sum() == 0, name
        elif name in KEEP_ALL:
            assert t.all(), name
        else:
            assert t.sum() > 0 and (valid & ~t).sum() > 0, (name, int(t.sum()), int((valid & ~t).sum()))
    # short lists both ways
    for name in ("i64_16", "s_16", "dec_other_scales", "ts_instants", "with_null", "minus_zero"):
        pred = cases()[name]
        a, b = mask(name), IM.evaluate(pred, table, leaf=IM.in_leaf_by_set, other=like_leaf)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all(), name
    # the tables on both sides of what is staged in LDS: 8 bytes a slot, twice the keys rounded up to a power of two
    assert 2 * 16 * 8 < 32768 < 8192 * 2 * 8 and len({v.value for v in cases()["i64_5000"].children}) > 4096


def expected_batches(table, keep, stripe_rows, batch_size, selection_batches=None):
    out, base = [], 0
    for k, n in enumerate(stripe_rows):
        idx = np.arange(base, base + n)
        if selection_batches is not None and selection_batches[k] is not None:
            idx = np.concatenate([np.arange(base + s, base + s + m) for s, m in selection_batches[k]] or [np.arange(0)]).astype(np.int64)
        kept = table.take(pa.array(idx[keep[idx]]))
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
    if pred is not None:
        b = b.with_row_filter(pred, prune=prune)
    if device:
        b = b.with_device_output()
    r = b.build()
    try:
        batches = [x.to_pyarrow() for x in r] if device else list(r)
        return batches, r.filter_rows(), r.row_groups()
    finally:
        r.close()


def same_column(a, b):
    """equal, a NaN being equal to a NaN"""
    one = lambda x: x if isinstance(x, pa.Array) else pa.concat_arrays(x.chunks) if x.num_chunks else pa.array([], x.type)
    a, b = one(a), one(b)
    a = a.cast(b.type)
    if not pa.types.is_floating(b.type):
        return a.equals(b)
    return a.is_valid().equals(b.is_valid()) and np.array_equal(a.fill_null(0).to_numpy(zero_copy_only=False), b.fill_null(0).to_numpy(zero_copy_only=False), equal_nan=True)


def same_batches(got, want, what):
    assert [b.num_rows for b in got] == [w.num_rows for w in want], what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.schema.names == w.schema.names, what
        g.validate(full=True)
        for name in w.schema.names:  # (column by column: a column whose kept rows hold no null is exported as not nullable)
            assert same_column(g.column(name), w.column(name)), what + (k, name)


def check(path, table, rows, pred, batch_size, keep, selection=None, **kw):
    sel_batches = M.file_batches(selection, rows, batch_size) if selection is not None else None
    want = expected_batches(table, keep, rows, batch_size, sel_batches)
    got, (seen, kept), groups = read(path, pred, batch_size=batch_size, selection=selection, **kw)
    same_batches(got, want, (os.path.basename(path), batch_size, kw))
    assert kept == sum(w.num_rows for w in want)
    return got, (seen, kept), groups


@pytest.mark.gpu
@pytest.mark.parametrize("compression", COMPRESSIONS)
@pytest.mark.parametrize("batch_size", BATCH_SIZES)
def test_every_case_against_the_model(tmpdir, batch_size, compression):
    """Every case with pruning off and on and with read-ahead 0 and 2 (which pairs with which alternates with the file), at both
    batch sizes; a list of at most 16 literals also against the reader's own OR of the EQ leaves."""
    path, table, rows = orc_file(tmpdir, compression)
    ways = ((False, 0), (True, 2)) if compression == "uncompressed" else ((False, 2), (True, 0))
    for name, pred in cases().items():
        t, _ = mask(name)
        for prune, prefetch in ways:
            got, (seen, kept), (read_groups, total_groups) = check(path, table, rows, pred, batch_size, t, prune=prune, prefetch=prefetch)
            assert kept == int(t.sum()) and (seen == N or prune), name
            assert prune or read_groups == total_groups
        if n_literals(pred) <= 16:
            other, (_, kept_or), _ = read(path, IM.or_of_eq(pred), batch_size=batch_size)
            same_batches(got, other, (name, "the OR of the EQ leaves"))
            assert kept_or == kept, name


@pytest.mark.gpu
@pytest.mark.parametrize("compression", COMPRESSIONS)
def test_under_a_row_selection_and_with_device_output(tmpdir, compression):
    path, table, rows = orc_file(tmpdir, compression)
    selections = [[(5, True), (60, False), (1000, True), (700, False), (2000, True), (300, False)], [(1, False), (4095, True), (1, False)],
                  [(100, True), (1, False), (63, True), (65, False)]]
    for name in ("i64_16", "i64_5000", "s_16", "s_5000", "i64_65536", "not_in_strings", "dec_other_scales", "two_tables_like", "bool_with_null", "with_null"):
        pred, (t, _) = cases()[name], mask(name)
        for batch_size in BATCH_SIZES:
            for sel in selections:
                check(path, table, rows, pred, batch_size, t, selection=sel)
            check(path, table, rows, pred, batch_size, t, device=True)
            check(path, table, rows, pred, batch_size, t, device=True, selection=selections[0], prune=True, prefetch=2)


@pytest.mark.gpu
def test_pruning_is_sound_and_reads_fewer_row_groups(tmpdir):
    """A sorted Int64 column with row groups of 1000 rows: a list inside one group reads fewer groups with prune=True and keeps
    the same rows; under a NOT nothing is pruned."""
    n = 6000
    table = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "v": pa.array(np.arange(n, dtype=np.int64) * 2)})
    path = str(tmpdir / "sorted.orc")
    orc.write_table(table, path, compression="uncompressed", stripe_size=64 << 20, row_index_stride=1000)
    rows = [orc.ORCFile(path).read_stripe(i).num_rows for i in range(orc.ORCFile(path).nstripes)]
    for vals in ([4200, 4202, 4201], [10, 1990], [1, 3, 5], list(range(4000, 4400))):  # (under a row filter the groups read are one run)
        pred = P.in_list("v", [V.Int64(x) for x in vals])
        keep = np.isin(np.arange(n) * 2, vals)
        _, (_, kept_f), (read_f, total_f) = check(path, table, rows, pred, 1000, keep, prune=False)
        _, (_, kept_t), (read_t, total_t) = check(path, table, rows, pred, 1000, keep, prune=True)
        assert kept_f == kept_t == int(keep.sum()) and read_f == total_f == total_t and read_t < read_f, vals
        _, _, (read_n, total_n) = check(path, table, rows, P.not_(pred), 1000, ~keep, prune=True)
        assert read_n == total_n


class RawNodes:
    """a node list as it is, where a Predicate is expected"""

    def __init__(self, nodes):
        self.nodes = nodes

    def flatten(self):
        keep, out = [], []
        for op, n_children, column, value in self.nodes:
            n = PR.PredicateNode()
            n.op, n.n_children = op, n_children
            if column is not None:
                keep.append(column.encode())
                n.column = keep[-1]
            if value is not None:
                n.value_type, n.i = PR.PV_INT64, value
            out.append(n)
        return (PR.PredicateNode * len(out))(*out), keep


def expect_refusal(builder, pred, code, word_):
    r = builder.with_row_filter(pred, prune=False).build()
    with pytest.raises(capi.OrcGpuError) as e:
        next(r)
    assert e.value.code == code and word_ in str(e.value), (code, word_, str(e.value))
    with pytest.raises(StopIteration):
        next(r)
    r.close()


@pytest.mark.gpu
def test_refusals_are_loud_and_name_the_column(tmpdir):
    path, table, rows = orc_file(tmpdir, "uncompressed")
    IN, LITERAL = PR.IN, PR.LITERAL
    for prefetch in (0, 2):
        new = lambda: ArrowReaderBuilder.try_new(path, ctx()).with_prefetch(prefetch)
        expect_refusal(new(), P.in_list("i64", [V.Int64(k) for k in range(65537)]), UNSUPPORTED, "'i64'")
        expect_refusal(new(), P.in_list("i64", [V.Int64(1), V.Utf8("a")]), MISMATCHED, "'i64'")
        expect_refusal(new(), P.in_list("s", [V.Utf8("a"), V.Int8(1)]), MISMATCHED, "'s'")
        expect_refusal(new(), P.in_list("dec", [V.Int64(1)]), UNSUPPORTED, "'dec'")
        expect_refusal(new(), P.in_list("ts", [V.TimestampNs(0), V.Int64(1)]), UNSUPPORTED, "'ts'")
        expect_refusal(new().with_dictionary_columns(["s"]), P.in_list("s", [V.Utf8("a"), V.Utf8("b")]), UNSUPPORTED, "'s'")
        expect_refusal(new().with_dictionary_columns(["s"]), P.in_list("s", [V.Utf8("a")]), UNSUPPORTED, "'s'")
        expect_refusal(new(), P.in_list("nope", [V.Int64(1)]), INVALID, "nope")
        # raw malformed node lists: a literal outside a list, a child that is no literal, a literal with children, a list cut short
        expect_refusal(new(), RawNodes([(LITERAL, 0, None, 1)]), INVALID, "literal")
        expect_refusal(new(), RawNodes([(PR.AND, 2, None, None), (PR.IS_NULL, 0, "i64", None), (LITERAL, 0, None, 1)]), INVALID, "literal")
        expect_refusal(new(), RawNodes([(IN, 2, "i64", None), (LITERAL, 0, None, 1), (PR.EQ, 0, "i64", 2)]), INVALID, "IN list")
        expect_refusal(new(), RawNodes([(IN, 2, "i64", None), (LITERAL, 1, None, 1), (LITERAL, 0, None, 2)]), INVALID, "children")
        expect_refusal(new(), RawNodes([(IN, 3, "i64", None), (LITERAL, 0, None, 1), (LITERAL, 0, None, 2)]), INVALID, "ends inside")
        expect_refusal(new(), RawNodes([(11, 0, "i64", 1)]), INVALID, "unknown node op")
    nested = str(tmpdir / "nested.orc")
    orc.write_table(pa.table({"v": pa.array([1, 2, None], pa.int64()), "l": pa.array([[1], [], None], pa.list_(pa.int32()))}), nested)
    expect_refusal(ArrowReaderBuilder.try_new(nested, ctx()), P.in_list("v", [V.Int64(1), V.Int64(5)]), UNSUPPORTED, "'l'")
    # ... and the context is as usable as before: the same files filter, 65536 literals are within the limit
    got, _, _ = read(nested, P.in_list("v", [V.Int64(2), V.Int64(5)]), names=["v"])
    assert [b.column("v").to_pylist() for b in got] == [[2]]
    check(path, table, rows, cases()["i64_65536"], 1000, mask("i64_65536")[0])
    # a list of only NULLs reads no value: the dictionary column is not refused, as EQ with the NULL literal is not
    got, (_, kept), _ = read(path, P.in_list("s", [V.Utf8(None)]), dictionary=["s"])
    assert got == [] and kept == 0


@pytest.mark.gpu
def test_in_is_new():
    """What the parent commit answers: op 17 is an unknown op (ORCGPU_INVALID_ARGUMENT) and Predicate.in_list does not exist."""
    assert PR.IN == 17 and PR.LITERAL == 18 and callable(P.in_list) and callable(P.not_in)
    from orc_rust_amd import gen
    ids = np.arange(5, dtype=np.int64)
    vals = np.array([10, 20, 30, 20, -1], dtype=np.int64)
    cols = [{"column_id": 1, "orc_type": 4, "encoding": 2}, {"column_id": 2, "orc_type": 4, "encoding": 2}]
    streams = [(1, 1, gen.rle2(ids, signed=True)), (2, 1, gen.rle2(vals, signed=True))]
    c = ctx()
    for pred, want in ((RawNodes([(PR.IN, 2, "v", None), (PR.LITERAL, 0, None, 20), (PR.LITERAL, 0, None, -1)]), [1, 3, 4]),
                       (P.not_in("v", [V.Int64(20), V.Int64(-1), V.Int64(7)]), [0, 2])):
        staged = c.stage(5, streams, cols, batch_size=64)
        res = c.decode([staged])[0]
        staged.free()
        assert c.result_filter(res, pred, ["id", "v"]) == len(want)
        res.fetch()
        assert res.export_batch(0).column(0).to_pylist() == want
        res.free()
