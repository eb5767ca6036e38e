"""agg(x) FILTER (WHERE p) on the GPU -- Agg.where, orcgpu_result_aggregate_filters, orcgpu_result_aggregate_groups_filters,
orcgpu_reader_set_aggregate_filters: agg_cond_eval_kernel and the condition planes every aggregate kernel honours -- against the
defining rule of include/orcgpu.h applied with the models the project has:

    a conditioned aggregate is the same aggregate computed as if its argument were NULL in every kept row for which the condition
    is not TRUE.

So for a spec with condition p the written table gets the spec's argument column(s) nulled where AM.kept_mask(table, p) is false
(the rows where p is TRUE under tests/in_model.py, filter_model_typed.py and like_model.py; COUNT_ROWS counts an all-valid column
nulled the same way), and that table goes to agg_model / agg_expr_model / group_model /
group_wide_model with the UNCONDITIONED spec and the same keep mask.  Expected values never come from a read of the file."""
import ctypes as C
import decimal
import os
import struct
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import agg_model as AM
import group_model as GM
import group_wide_model as WM
import in_model as IM
import like_model as LM
import test_gpu_aggregate as TA
import test_gpu_aggregate_expr as TX
from orc_rust_amd import aggregate as A
from orc_rust_amd import capi
from orc_rust_amd import predicate as PR
from orc_rust_amd.aggregate import Agg, col
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V

pytestmark = pytest.mark.gpu

D = decimal.Decimal
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, INVALID = 7, 101
NAMES = ["id", "g", "i8", "i32", "i64", "f32", "f64", "dec", "s", "k256"]
_T, _F, _PASS = {}, {}, {}


def table_of(n):
    """TA.make_table(n, 0.3) cut to NAMES, with k256 = a key of 256 groups whose first appearances are not in key order"""
    if n not in _T:
        t = TA.make_table(n, 0.3)
        k = (np.arange(n, dtype=np.int64) * 37) % 256
        _T[n] = t.select([c for c in NAMES if c != "k256"]).append_column("k256", pa.array(k, pa.int64()))
    return _T[n]


def file_of(n, stripes=1):
    if (n, stripes) not in _F:
        _F[(n, stripes)] = TA.own_file(table_of(n), stripes=stripes)[0]
    return _F[(n, stripes)]


# ---- the conditions: always TRUE, always FALSE, a comparison on a nullable column and its NOT (both exclude the UNKNOWN rows),
# a LIKE, an IN with a NULL literal (no row is FALSE under it), and -- per aggregate -- one on the aggregated column itself
TRUE, FALSE = P.is_not_null("id"), P.is_null("id")
CMP = P.gt("i32", V.Int32(0))
LIKE = P.like("s", "row 1%")
IN_NULL = P.in_list("i8", [V.Int8(v) for v in range(-40, 40, 3)] + [V.Int8(None)])
SELF = {"s": P.gt("s", V.Utf8("row 5")), "i64": P.gt("i64", V.Int64(0)), "i32": P.lte("i32", V.Int32(1000)), "i8": P.ne("i8", V.Int8(0)),
        "dec": P.lt("dec", V.Decimal128(D("0.00"))), "f64": P.gte("f64", V.Float64(0.0)), "f32": P.lt("f32", V.Float32(50.0)), None: P.is_not_null("i64")}


def conditions(arg):
    return [None, TRUE, FALSE, CMP, P.not_(CMP), LIKE, IN_NULL, SELF[arg]]


DISC = col("dec") * (1 - col("dec"))
# (the aggregate, the column its own-column condition is on): every op and kind
OPS = [(Agg.count_rows(), None), (Agg.count("s"), "s"), (Agg.sum("i64"), "i64"), (Agg.sum("dec"), "dec"), (Agg.sum("f64"), "f64"),
       (Agg.min("i32"), "i32"), (Agg.max("i32"), "i32"), (Agg.min("dec"), "dec"), (Agg.max("dec"), "dec"), (Agg.min("f64"), "f64"), (Agg.max("f64"), "f64"),
       (Agg.sum_product("i8", "i64"), "i8"), (Agg.sum_product("f32", "f64"), "f32"), (Agg.sum(DISC), "dec"), (Agg.avg(col("i32") * col("i8")), "i32"),
       (Agg.avg("dec"), "dec"), (Agg.avg("f64"), "f64"), (Agg.sum(col("f64") * col("f32") + 0.5), "f64")]
ONE_OF_EACH = [OPS[k] for k in (0, 2, 3, 4, 8, 9, 13, 16)]      # above 1025 rows: one column of each kind


def crossed(ops):
    """every aggregate of `ops` unconditioned and under each condition, cut into lists of at most 64 specs: every list holds the
    same aggregate unconditioned and conditioned several ways, and several aggregates that share one condition"""
    per = A.AGG_MAX // 8
    return [[a if p is None else a.where(p) for a, arg in ops[k:k + per] for p in conditions(arg)] for k in range(0, len(ops), per)]


def _leaf(pred, table):
    """a LIKE leaf by tests/like_model.py, every other leaf by the typed filter model: (TRUE rows, FALSE rows)"""
    if pred.op != PR.LIKE:
        return IM.FMT.evaluate(pred, table)
    got = LM.like_column(table.column(pred.column).to_pylist(), pred.value.value, pred.escape)
    return np.array([g is True for g in got], bool), np.array([g is False for g in got], bool)


def passes(table, p):
    """AM.kept_mask(table, p) for a condition -- the rows where it is TRUE --, with the LIKE leaves the filter models leave to like_model"""
    key = (id(table), id(p))
    if key not in _PASS or _PASS[key][0] is not table or _PASS[key][1] is not p:     # (both are held: their ids are not given out again)
        _PASS[key] = (table, p, IM.evaluate(p, table, other=_leaf)[0])
    return _PASS[key][2]


def plain_of(spec):
    return Agg(spec.op, spec.column, spec.column2, spec.expr)


def nulled(table, spec):
    """the rule: (the table with the spec's argument nulled where its condition is not TRUE, the unconditioned spec)"""
    if spec.filter is None:
        return table, spec
    ok = pa.array(passes(table, spec.filter))
    if spec.op == A.COUNT_ROWS:
        names, plain = ["id"], Agg.count("id")
    else:
        names = [c for c in (spec.column, spec.column2) if c is not None] + ([x.column for x in TX.XM.leaves(spec.expr) if x.op == A.EXPR_COLUMN] if spec.expr is not None else [])
        plain = plain_of(spec)
    for name in dict.fromkeys(names):
        c = table.column(name)
        table = table.set_column(table.column_names.index(name), name, pc.if_else(ok, c, pa.scalar(None, c.type)))
    return table, plain


def check(table, specs, got, keep, what):
    for s, g in zip(specs, got):
        t2, s2 = nulled(table, s)
        TX.check(t2, [s2], [g], keep, (what, s))


def check_groups(table, specs, group_by, got, keep, what, f64_bits=None):
    """groups and order from the kept rows alone; the values per group by the rule.  f64_bits: {spec index: raw record list} whose
    Double sums are held bit for bit to the wide path's fold rule (tests/group_wide_model.py) on the nulled table."""
    want = GM.group_rows(table, group_by, keep)
    assert [tuple(GM.key_id(k) for k in keys) for keys, _ in got] == [tuple(GM.key_id(k) for k in keys) for keys, _ in want], what
    for k, s in enumerate(specs):
        t2, s2 = nulled(table, s)
        vals = t2.column(s2.column).to_pylist() if f64_bits is not None and k in f64_bits else None
        for g, ((keys, out), (_, mask)) in enumerate(zip(got, want)):
            sub = t2.filter(pa.array(mask))
            TX.check(sub, [s2], [out[k]], np.ones(sub.num_rows, bool), (what, keys, s))
            if vals is not None:
                fold, count = WM.fold_f64([vals[r] for r in np.flatnonzero(mask)])
                rec = f64_bits[k][g]
                assert (rec.is_null, struct.pack("<d", rec.f)) == (int(count == 0), struct.pack("<d", fold if count else 0.0)), (what, keys, s, rec.f, fold)


def run_groups(src, specs, group_by, max_groups=None, **kw):
    r = TA.builder(src, NAMES, **kw).aggregating_reader(specs, group_by=group_by, max_groups=max_groups)
    try:
        raw = r.aggregate(raw=True)
        return raw, [(keys, [AM.OVERFLOW if v.overflow else A.value_of(v, s) for v, s in zip(vals, specs)]) for keys, vals in raw], r.filter_rows(), r.d2h_bytes()
    finally:
        r.close()


# ---- ungrouped: every size x kept-row arm x condition x op ----
@pytest.mark.parametrize("n", TA.SIZES)
def test_every_size_arm_condition_and_op(n):
    table, data = table_of(n), file_of(n)
    # every condition at every size.  Above 1025 rows one column of each kind; at 70 001 rows the six of them that are no expression
    # and no average (those are held to the model under every condition up to 2049 rows: the model of an expression walks every row
    # in Python, per spec) and two arms -- no filter, and the IN filter under a row selection
    lists = crossed(OPS if n <= 1025 else ONE_OF_EACH if n < 70_001 else ONE_OF_EACH[:6])
    arms = TA.arms(n) if n < 70_001 else [TA.arms(n)[0], TA.arms(n)[4]]
    for name, pred, sel in arms:
        if n == 0 and sel is not None:
            sel = [(5, True), (5, False)]
        keep = AM.kept_mask(table, pred, sel, TA.BATCH)
        for specs in lists:
            got, (seen, kept), d2h = TA.run(data, NAMES, specs, pred=pred, selection=sel)
            check(table, specs, got, keep, (n, name))
            # the kept rows are the selection's and the row filter's: conditions change neither them nor the bytes copied back
            assert (seen, kept, d2h) == (int(AM.kept_mask(table, None, sel, TA.BATCH).sum()), int(keep.sum()), 0), (n, name)


def records(raw):
    return [(v.kind, v.is_null, v.overflow, v.scale_or_unit, tuple(v.w), struct.pack("<d", v.f)) for v in raw]


@pytest.mark.parametrize("n", (1025, 70_001))
def test_a_condition_is_the_row_filter_and_ed_with_it_bit_for_bit(n):
    data = file_of(n)
    plain = [a for a, _ in OPS]
    for f in (None, P.lt("g", V.Int64(1)), P.in_list("g", [V.Int64(-2), V.Int64(0), V.Int64(3)])):
        for p in (CMP, P.not_(CMP), LIKE, IN_NULL, FALSE):
            cond = TA.builder(data, NAMES, pred=f).aggregate([a.where(p) for a in plain], raw=True)
            both = TA.builder(data, NAMES, pred=P.and_([f, p] if f is not None else [p])).aggregate(plain, raw=True)
            assert records(cond) == records(both), (n, p)           # the AND-ed masks are the same words: Double sums included


# ---- grouped, both paths ----
GROUP_OPS = [OPS[k] for k in (0, 1, 2, 3, 4, 6, 9, 13, 16)]
GONE = P.ne("g", V.Int64(2))        # no row of the group g = 2 passes


def group_specs():
    specs = [a if p is None else a.where(p) for a, arg in GROUP_OPS for p in (None, GONE, CMP, LIKE, SELF[arg])]
    return specs + [Agg.count_rows().where(IN_NULL), Agg.sum("f64").where(P.not_(CMP)), Agg.sum("f64").where(FALSE), Agg.sum("f64").where(TRUE)]


@pytest.mark.parametrize("max_groups", (None, 257))          # the narrow path; a limit above 256 forces the wide one
@pytest.mark.parametrize("n", (65, 1025, 2049))
def test_groups_exist_by_their_kept_rows_whatever_the_conditions_say(n, max_groups):
    table, data = table_of(n), file_of(n)
    specs = group_specs()
    f64 = [k for k, s in enumerate(specs) if s.op == A.SUM and s.column == "f64"]
    for name, pred, sel in TA.arms(n) if n <= 1025 else TA.arms(n)[::2]:
        keep = AM.kept_mask(table, pred, sel, TA.BATCH)
        raw, got, (_, kept), d2h = run_groups(data, specs, ["g"], max_groups, pred=pred, selection=sel)
        bits = {k: [vals[k] for _, vals in raw] for k in f64} if max_groups else None
        check_groups(table, specs, ["g"], got, keep, (n, name, max_groups), bits)
        assert (kept, d2h) == (int(keep.sum()), 0)
        # the group none of whose rows pass is there, in its first-appearance place, with NULL -- or 0 for the counts
        for keys, vals in got:
            if keys == (2,):
                assert vals[1] == 0 and vals[11] is None and vals[0] > 0, (n, name, vals[:12])     # count_rows / sum('i64') under GONE; the plain count_rows
        assert any(keys == (2,) for keys, _ in got) == bool((keep & (table.column("g").to_numpy() == 2)).any())


@pytest.mark.parametrize("max_groups", (None, 257))
def test_256_groups_and_a_one_bit_hash(monkeypatch, max_groups):
    n = 2049
    table, data = table_of(n), file_of(n)
    specs = [Agg.count_rows(), Agg.count_rows().where(CMP), Agg.sum("f64").where(LIKE), Agg.sum("f64"), Agg.sum("dec").where(SELF["dec"]), Agg.max("i32").where(IN_NULL),
             Agg.avg("f64").where(CMP), Agg.sum(DISC).where(P.not_(CMP))]
    pred = P.gte("id", V.Int64(3))
    keep = AM.kept_mask(table, pred)
    raw, got, _, d2h = run_groups(data, specs, ["k256"], max_groups, pred=pred)
    assert len(got) == 256 and d2h == 0
    check_groups(table, specs, ["k256"], got, keep, ("256 groups", max_groups), {k: [vals[k] for _, vals in raw] for k in (2, 3)} if max_groups else None)
    monkeypatch.setenv("ORCGPU_GROUP_HASH_BITS", "1")           # two hash values for 256 keys: the longest probe sequences
    again, _, _, _ = run_groups(data, specs, ["k256"], max_groups, pred=pred)
    assert [(k, records(v)) for k, v in again] == [(k, records(v)) for k, v in raw]


# ---- the reader: several stripes ----
def test_reader_merges_the_stripes_and_reports_the_kept_rows_as_without_conditions():
    n = 3 * 1025 + 7
    table, data = table_of(n), file_of(n, stripes=3)
    specs = crossed(ONE_OF_EACH)[0]
    pred = P.lt("g", V.Int64(1))
    keep = AM.kept_mask(table, pred)
    for prefetch in (0, 2):
        got, rows, d2h = TA.run(data, NAMES, specs, pred=pred, prefetch=prefetch)
        exact = [(s, g) for s, g in zip(specs, got) if not isinstance(g, float)]
        check(table, [s for s, _ in exact], [g for _, g in exact], keep, ("stripes", prefetch))
        _, rows_plain, _ = TA.run(data, NAMES, [plain_of(s) for s in specs], pred=pred, prefetch=prefetch)
        assert rows == rows_plain == (n, int(keep.sum())) and d2h == 0
    # a Double sum over three stripes is the stripes' sums added in stripe order: within the bound of any order
    floats = [(s, g) for s, g in zip(specs, got) if isinstance(g, float)]
    check(table, [s for s, _ in floats], [g for _, g in floats], keep, "stripes, doubles")
    for max_groups in (None, 257):
        gspecs = group_specs()[:20]
        _, groups, rows, d2h = run_groups(data, gspecs, ["g"], max_groups, pred=pred, prefetch=2)
        check_groups(table, gspecs, ["g"], groups, keep, ("stripes grouped", max_groups))
        assert rows == (n, int(keep.sum())) and d2h == 0


# ---- nothing may depend on what the workspace held ----
CHILD = r'''
import sys
sys.path[:0] = [%r, %r]
import torch
import test_gpu_aggregate_filter as T
n = 2049
data = T.file_of(n)
specs = T.group_specs()
out = []
for _ in range(2):      # (the second call reuses the workspace: what POISON is about)
    for pred in (None, T.P.lt("g", T.V.Int64(1))):
        out.append(T.records(T.TA.builder(data, T.NAMES, pred=pred).aggregate(specs, raw=True)))
        for max_groups in (None, 257):
            raw = T.TA.builder(data, T.NAMES, pred=pred).aggregate(specs, raw=True, group_by=["k256"], max_groups=max_groups)
            out.append([(k, T.records(v)) for k, v in raw])
print("ANSWER", repr(out))
'''


def test_poison_does_not_show_through_the_planes():
    lines = []
    for extra in ({}, {"ORCGPU_POISON": "0xFF"}):
        env = {k: v for k, v in os.environ.items() if not k.startswith("ORCGPU_")}
        env.update(extra)
        p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-3000:]      # (a child that faults fails here: no further child is started)
        lines.append([ln for ln in p.stdout.decode().splitlines() if ln.startswith("ANSWER")][-1])
    assert lines[0] == lines[1] and len(lines[0]) > 10_000


# ---- refusals ----
def test_refusals_are_the_row_filters():
    n = 1025
    data = file_of(n)
    for group_by in (None, ["g"]):
        r = TA.builder(data, ["id", "g", "i64"]).aggregating_reader([Agg.sum("i64").where(P.gt("i32", V.Int32(0)))], group_by=group_by)     # not projected
        with pytest.raises(capi.OrcGpuError) as e:
            r.aggregate()
        assert e.value.code == INVALID and "'i32'" in str(e.value) and "row filter" in str(e.value)
        r.close()
        r = TA.builder(data, NAMES).with_dictionary_columns(["s"]).aggregating_reader([Agg.count_rows().where(LIKE)], group_by=group_by)
        with pytest.raises(capi.OrcGpuError) as e:
            r.aggregate()
        assert e.value.code == UNSUPPORTED and "'s'" in str(e.value) and "dictionary" in str(e.value)
        r.close()
    # IS NULL reads the validity alone: allowed on a dictionary column, as under the row filter
    got = TA.builder(data, NAMES).with_dictionary_columns(["s"]).aggregate([Agg.count_rows().where(P.is_null("s")), Agg.count("s")])
    assert got[0] + got[1] == n
    # orcgpu_reader_set_aggregate_filters: n_specs must be the list's; before set_aggregates there is no list
    b = TA.builder(data, NAMES)
    L = TA.ctx().L
    specs = [Agg.count_rows().where(CMP), Agg.sum("i64")]
    filters, keep = A.filter_array(specs)
    arr, keep_s = A.spec_array(specs)
    assert L.orcgpu_reader_set_aggregate_filters(b._h, filters, 2) == INVALID
    assert L.orcgpu_reader_set_aggregates(b._h, arr, 2) == 0
    assert L.orcgpu_reader_set_aggregate_filters(b._h, filters, 1) == INVALID
    assert L.orcgpu_reader_set_aggregate_filters(b._h, filters, 3) == INVALID
    r = b.build()
    r._agg_specs, r._group_by = specs, None
    table = table_of(n)
    assert r.aggregate() == [n, AM.aggregate(table, [Agg.sum("i64")])[0]]       # nothing changed: no condition was set
    r.close()
    b = TA.builder(data, NAMES)
    assert L.orcgpu_reader_set_aggregates(b._h, arr, 2) == 0 and L.orcgpu_reader_set_aggregate_filters(b._h, filters, 2) == 0
    r = b.build()
    r._agg_specs, r._group_by = specs, None
    assert r.aggregate() == [int(passes(table, CMP).sum()), AM.aggregate(table, [Agg.sum("i64")])[0]]
    r.close()


# ---- filters = NULL is the older entry point ----
def test_no_condition_through_the_new_entry_points_is_the_old_answer():
    res, table = TA.stripe_result(4097)
    c = TA.ctx()
    specs = [Agg.count_rows(), Agg.count("v"), Agg.sum("v"), Agg.min("v"), Agg.max("v"), Agg.sum_product("v", "id"), Agg.avg("v"), Agg.sum(col("v") * col("id") - 1)]
    pred = P.gt("v", V.Int64(10))
    for p in (None, pred):
        rows, (arr, exprs, filters, n), keep = c._aggregate_args(specs, ["id", "v"], p)
        assert filters is None
        old, new, empty = (A.AggValue * n)(), (A.AggValue * n)(), (A.AggValue * n)()
        assert c.L.orcgpu_result_aggregate_exprs(c.h, res.h, *rows, arr, exprs, n, old) == 0
        assert c.L.orcgpu_result_aggregate_filters(c.h, res.h, *rows, arr, exprs, None, n, new) == 0
        assert c.L.orcgpu_result_aggregate_filters(c.h, res.h, *rows, arr, exprs, (A.AggFilter * n)(), n, empty) == 0      # {NULL, 0} everywhere
        assert records(old) == records(new) == records(empty)
        assert A.values_of(new, specs) == [TX.want_of(table, s, AM.kept_mask(table, p)) for s in specs]
        keys = A.key_array(["v"])
        for max_groups in (0, 300):
            out_old, out_new = C.c_void_p(), C.c_void_p()
            assert c.L.orcgpu_result_aggregate_groups_limit(c.h, res.h, *rows, keys, 1, arr, exprs, n, max_groups, C.byref(out_old)) == 0
            assert c.L.orcgpu_result_aggregate_groups_filters(c.h, res.h, *rows, keys, 1, arr, exprs, None, n, max_groups, C.byref(out_new)) == 0
            a, b = A.groups_of(c.L, out_old, 1, specs, raw=True), A.groups_of(c.L, out_new, 1, specs, raw=True)
            assert [(k, records(v)) for k, v in a] == [(k, records(v)) for k, v in b] and len(a) > 30
    # ... and with conditions the result-level calls give what the reader gives
    cond = [s.where(P.lt("id", V.Int64(2000))) for s in specs]
    got = c.result_aggregate(res, cond, ["id", "v"])
    check(table, cond, got, np.ones(4097, bool), "result level")
    grouped = c.result_aggregate_groups(res, cond, ["v"], ["id", "v"], max_groups=300)
    check_groups(table, cond, ["v"], grouped, np.ones(4097, bool), "result level, wide")
    res.free()
