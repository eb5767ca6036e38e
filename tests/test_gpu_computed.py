"""Computed columns on the GPU (ArrowReaderBuilder.with_computed_columns; compute_columns_kernel in device/compute_kernels.hip,
launched inside the decode call) against tests/computed_model.py, row for row and exactly: integers and Decimals as Python ints,
doubles by their bits.  Files are written in the test with pyarrow (this library's writer takes no Date), one stripe or four, a
few thousand rows at most.  Every test here needs with_computed_columns: none passes without the feature."""
import decimal

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import agg_expr_model as AEM
import computed_model as M
import test_gpu_aggregate as TA
import top_k_model as TK
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg, col, lit
from orc_rust_amd.arrow_reader import ArrowReaderBuilder, concat_batches
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
from orc_rust_amd.top_k import SortKey

pytestmark = pytest.mark.gpu

D = decimal.Decimal
EXACT = decimal.Context(prec=80)


def dec(unscaled, scale):
    """the Decimal of an unscaled int at a scale, exactly (the default context rounds to 28 digits)"""
    return D(unscaled).scaleb(-scale, EXACT)

BATCH = 1024
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63
SCHEMA = {"id": "int", "g": "int", "i8": "int", "i16": "int", "i32": "int", "a": "int", "b": "int", "nn": "int", "allnull": "int", "dt": "date",
          "p": ("dec", 2), "q": ("dec", 4), "w": ("dec", 0), "x": "float", "y": "float", "xi": "float", "s": "string"}
ARROW = {"id": pa.int64(), "g": pa.int32(), "i8": pa.int8(), "i16": pa.int16(), "i32": pa.int32(), "a": pa.int64(), "b": pa.int64(), "nn": pa.int64(), "allnull": pa.int64(),
         "dt": pa.date32(), "p": pa.decimal128(12, 2), "q": pa.decimal128(20, 4), "w": pa.decimal128(38, 0), "x": pa.float64(), "y": pa.float64(), "xi": pa.float64(), "s": pa.string()}
EXPRS = {
    "isum": col("a") + col("b"),                       # Int64; overflows at the int64 edges
    "imix": col("i8") * col("i16") - col("i32") + col("dt"),  # Byte / Short / Int / Date operands
    "ineg": -col("a"),                                 # -(-2^63) does not fit
    "inn": col("nn") * 3 + 1,                          # no NULL at all (no PRESENT stream)
    "inull": col("allnull") + col("id"),               # an operand all NULL
    "drev": col("p") * (1 - col("q")),                 # Decimal, scales 2 and 4 -> 6
    "dwide": col("w") * col("w"),                      # reaches 10^38 and leaves 128 bits
    "fsum": col("x") * col("y") + 0.5,                 # Float64, rounded after every operation
}
_CTX = None


def ctx():
    global _CTX
    if _CTX is None:
        _CTX = capi.Context()
    return _CTX


def make_columns(n, seed=5):
    """name -> a list of the model's values (ints, unscaled ints, floats; None: NULL).  NULLs at word edges (rows 0, 63, 64, 127, 128)"""
    rng = np.random.default_rng(seed + n)

    def nulls(values, frac=0.2):
        out = [None if m else v for v, m in zip(values, rng.random(n) < frac)]
        for edge in (0, 63, 64, 127, 128, n - 1):
            if 0 <= edge < n:
                out[edge] = None if edge % 2 == 0 else values[edge]
        return out

    def pick(pool):
        return [pool[int(k) % len(pool)] for k in rng.integers(0, 1 << 30, n)]

    c = {"id": list(range(n)), "nn": [int(v) for v in rng.integers(-1000, 1000, n)], "allnull": [None] * n}
    c["g"] = nulls([int(v) for v in rng.integers(0, 20, n)])
    c["i8"] = nulls([int(v) for v in rng.integers(-128, 128, n)])
    c["i16"] = nulls([int(v) for v in rng.integers(-32768, 32768, n)])
    c["i32"] = nulls([int(v) for v in rng.integers(-2 ** 31, 2 ** 31, n)])
    c["a"] = nulls(pick([I64_MAX, I64_MIN, 0, 1, -1, 17, I64_MAX - 1, I64_MIN + 1, 5, 5, 7]))
    c["b"] = nulls(pick([1, -1, 0, I64_MAX, I64_MIN, 2, 5, 5]))
    c["dt"] = nulls([int(v) for v in rng.integers(-1000, 20000, n)])
    c["p"] = nulls(pick([150, 199, -1, 0, 10 ** 12 - 1, 1 - 10 ** 12, 5, 100]))
    c["q"] = nulls(pick([500, 0, 10000, -2500, 10 ** 20 - 1, 1 - 10 ** 20, 700]))
    c["w"] = nulls(pick([10 ** 19, 10 ** 19 - 1, -(10 ** 19), 3, 0, 10 ** 38 - 1, 1 - 10 ** 38, 2 ** 64, 10 ** 18]))
    floats = [0.1, 0.2, -0.0, 0.0, 1.5, float("nan"), float("inf"), -float("inf"), 1e308, 10.0, 1e-320, 0.30000000000000004]
    c["x"] = nulls(pick(floats))
    c["y"] = nulls(pick(floats))
    c["xi"] = nulls([float(v) / 2 for v in rng.integers(-2000, 2000, n)])  # (halves: every sum of them is exact in any order)
    c["s"] = ["s%d" % (k % 7) for k in range(n)]
    return c


def arrow_table(c, names):
    arrays = []
    for name in names:
        t = SCHEMA[name]
        if isinstance(t, tuple):
            arrays.append(pa.array([None if v is None else dec(v, t[1]) for v in c[name]], ARROW[name]))
        else:
            arrays.append(pa.array(c[name], ARROW[name]))
    return pa.table(arrays, names=names)


def write_stripes(path, table, stripes):
    """`table` as an ORC file: one stripe, or -- stripes > 1, under a tiny stripe_size -- stripes of 1024 rows each but the last"""
    orc.write_table(table, path, compression="uncompressed", row_index_stride=1000, stripe_size=(64 << 20) if stripes == 1 else 1024)
    assert stripes == 1 or orc.ORCFile(path).nstripes == (table.num_rows + 1023) // 1024
    return path


class File:
    def __init__(self, tmpdir, n, stripes=3, names=None):
        self.n = n
        self.names = names or list(SCHEMA)
        self.c = make_columns(n)
        self.rows = [{k: self.c[k][i] for k in self.names} for i in range(n)]
        self.path = write_stripes(str(tmpdir / ("c%d.orc" % n)), arrow_table(self.c, self.names), stripes)

    def builder(self, exprs, prefetch=0):
        return ArrowReaderBuilder.try_new(self.path, ctx()).with_batch_size(BATCH).with_prefetch(prefetch).with_computed_columns(exprs)

    def model(self, name):
        return M.eval_column(EXPRS[name], SCHEMA, self.rows)


def got_values(table, name):
    """the column as the model spells it: ints, a Decimal's unscaled int, a double's bits"""
    colm = table.column(name)
    t = colm.type
    out = []
    for v in colm.to_pylist():
        if v is None:
            out.append(None)
        elif pa.types.is_decimal(t):
            out.append(int(v.scaleb(t.scale, EXACT)))
        elif pa.types.is_floating(t):
            out.append(M.bits(v))
        else:
            out.append(v)
    return out


def want_values(name, values):
    kind, _ = M.output_type(EXPRS[name], SCHEMA)
    return [M.bits(v) for v in values] if kind == M.FLOAT64 else values


def arrow_type_of(name):
    kind, s = M.output_type(EXPRS[name], SCHEMA)
    return pa.int64() if kind == M.INT64 else pa.float64() if kind == M.FLOAT64 else pa.decimal128(38, s)


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    return File(tmp_path_factory.mktemp("computed"), 3 * 1024 + 65)  # four stripes: three of a whole batch, one of a word and a row


@pytest.mark.parametrize("n, stripes", [(1, 1), (63, 1), (64, 1), (65, 1), (255, 1), (257, 1), (1025, 1), (1025, 2), (2049, 3)])
def test_rows_against_the_model(tmp_path, n, stripes):
    f = File(tmp_path, n, stripes=stripes)  # (stripes > 1: of 1024 rows each, the last of ONE row)
    names = list(EXPRS)  # eight computed columns at once
    reader = f.builder([(k, EXPRS[k]) for k in names]).build()
    batches = list(reader)
    for b in batches:
        b.validate(full=True)
        assert b.schema.names == f.names + names
        for k in names:
            fld = b.schema.field(k)
            assert fld.nullable and fld.type == arrow_type_of(k), (k, fld)
    table = concat_batches(batches)
    assert table.num_rows == n
    over = 0
    for k in names:
        want, o = f.model(k)
        over += o
        assert got_values(table, k) == want_values(k, want), k
    assert reader.computed_overflow_rows() == over
    assert reader.column_names() == f.names + names
    # the file's own columns are what a reader without computed columns hands out
    plain = concat_batches(list(ArrowReaderBuilder.try_new(f.path, ctx()).with_batch_size(BATCH).with_prefetch(0).build()))
    for name in f.names:
        assert got_values(table, name) == got_values(plain, name), name


def test_overflow_kinds_are_null_and_counted(big):
    for k in ("isum", "ineg", "dwide"):
        want, over = big.model(k)
        assert over > 0, k
        reader = big.builder({k: EXPRS[k]}).build()
        table = concat_batches(list(reader))
        assert got_values(table, k) == want
        assert reader.computed_overflow_rows() == over
    # the three kinds are all in the data: an operation leaving 128 bits, an Int64 result past int64, a Decimal reaching 10^38
    rows = big.rows
    assert any(r["w"] is not None and abs(r["w"]) == 2 ** 64 for r in rows)
    assert any(r["w"] is not None and abs(r["w"]) == 10 ** 19 for r in rows)
    assert any(r["a"] == I64_MAX and r["b"] == 1 for r in rows)


def test_poison_and_read_ahead(big, monkeypatch):
    monkeypatch.setenv("ORCGPU_POISON", "0xA5")  # a value or validity word left unwritten shows
    for prefetch in (0, 2):
        reader = big.builder([(k, EXPRS[k]) for k in EXPRS], prefetch=prefetch).build()
        table = concat_batches(list(reader))
        for k in EXPRS:
            assert got_values(table, k) == want_values(k, big.model(k)[0]), (k, prefetch)


def test_selection_and_row_filter(big):
    sel = [(100, True), (30, False), (900, True), (70, False), (1200, True), (500, False), (337, True)]  # (to the file's end: behind a selection's end stripes are read whole)
    picked = np.zeros(big.n, bool)
    at = 0
    for count, skip in sel:
        if not skip:
            picked[at:at + count] = True
        at += count
    names = ["isum", "dwide", "fsum"]
    kept_f = np.array([r["id"] % 3 == 0 for r in big.rows])
    pred = P.in_list("id", [V.Int64(k) for k in range(0, big.n, 3)])
    for use_sel, use_filter in ((True, False), (False, True), (True, True)):
        for prune in (True, False):
            b = big.builder([(k, EXPRS[k]) for k in names]).with_row_group_pruning(prune)
            keep = np.ones(big.n, bool)
            if use_sel:
                b = b.with_row_selection(sel)
                keep &= picked
            if use_filter:
                b = b.with_row_filter(pred, prune=prune)
                keep &= kept_f
            reader = b.build()
            table = concat_batches(list(reader))
            assert table.column("id").to_pylist() == [i for i in range(big.n) if keep[i]]
            over = 0
            for k in names:
                want = [v for v, ok in zip(want_values(k, big.model(k)[0]), keep) if ok]
                assert got_values(table, k) == want, (k, use_sel, use_filter, prune)
                # the count: of the selected rows, before the filter -- whatever row groups were read to get them
                counted = picked if use_sel else np.ones(big.n, bool)
                over += sum(1 for i, r in enumerate(big.rows) if counted[i] and M.eval_value(EXPRS[k], SCHEMA, r)[1])
            assert over > 0 and reader.computed_overflow_rows() == over, (use_sel, use_filter, prune)


def test_row_filter_leaves_on_a_computed_column(big):
    want, _ = big.model("imix")
    some = sorted({v for v in want if v is not None})[:40]
    cases = [  # (the predicate, what the model keeps of row i with value v)
        (P.gt("imix", V.Int64(0)), lambda i, v: v is not None and v > 0),
        (P.between("imix", V.Int64(-2 ** 30), V.Int64(2 ** 30)), lambda i, v: v is not None and -2 ** 30 <= v <= 2 ** 30),
        (P.in_list("imix", [V.Int64(v) for v in some]), lambda i, v: v in some),
        (P.compare(col("imix") + col("id"), "<", lit(5000)), lambda i, v: v is not None and v + i < 5000),
        (P.is_null("imix"), lambda i, v: v is None),
    ]
    for pred, ok in cases:
        exp = [i for i in range(big.n) if ok(i, want[i])]
        assert exp, pred
        for prune in (True, False):  # as a pruning predicate it keeps every row group: the same rows
            b = big.builder({"imix": EXPRS["imix"]}).with_row_filter(pred, prune=prune)
            batches = list(b.build())
            got = concat_batches(batches).column("id").to_pylist() if batches else []
            assert got == exp, (pred, prune)
    # Decimal and Double leaves
    wd, _ = big.model("drev")
    t = concat_batches(list(big.builder({"drev": EXPRS["drev"]}).with_row_filter(P.compare(col("drev"), ">", lit(0)), prune=False).build()))
    assert t.column("id").to_pylist() == [i for i in range(big.n) if wd[i] is not None and wd[i] > 0]
    wf, _ = big.model("fsum")
    t = concat_batches(list(big.builder({"fsum": EXPRS["fsum"]}).with_row_filter(P.gt("fsum", V.Float64(0.5)), prune=False).build()))
    assert t.column("id").to_pylist() == [i for i in range(big.n) if wf[i] is not None and wf[i] > 0.5]


def test_in_set_and_collect_keys(big):
    want, _ = big.model("imix")
    small = [i for i in range(big.n) if i % 5 == 0]
    ks = big.builder({"imix": EXPRS["imix"]}).with_row_filter(P.in_list("id", [V.Int64(i) for i in small]), prune=False).collect_keys("imix", max_keys=1 << 12)
    try:
        keys = {want[i] for i in small if want[i] is not None}
        assert len(ks) == len(keys)
        t = concat_batches(list(big.builder({"imix": EXPRS["imix"]}).with_row_filter(P.in_set("imix", ks), prune=False).build()))
        assert t.column("id").to_pylist() == [i for i in range(big.n) if want[i] in keys]
    finally:
        ks.close()


AGG_EXPRS = {"imix": EXPRS["imix"], "drev": EXPRS["drev"], "fint": col("xi") * 2.0, "gk": col("g") + 100, "gd": col("p") * 2}


def model_aggregates(big, rows_idx):
    """what AGG_SPECS give over the rows rows_idx, by the model: exact ints, Decimals, and doubles whose sums are exact"""
    vals = {k: M.eval_column(AGG_EXPRS[k], SCHEMA, [big.rows[i] for i in rows_idx])[0] for k in ("imix", "drev", "fint")}
    vi = [v for v in vals["imix"] if v is not None]
    vd = [v for v in vals["drev"] if v is not None]
    vf = [v for v in vals["fint"] if v is not None]
    avg_d = AEM.avg_decimal(sum(vd), len(vd), 6) if vd else None
    return [len(rows_idx), len(vi), sum(vi) if vi else None, min(vi) if vi else None, max(vi) if vi else None, AEM.avg_int(sum(vi), len(vi)) if vi else None,
            dec(sum(vd), 6) if vd else None, dec(min(vd), 6) if vd else None, dec(max(vd), 6) if vd else None, dec(*avg_d) if vd else None,
            len(vf), sum(vf) if vf else None, min(vf) if vf else None, max(vf) if vf else None, sum(vf) / len(vf) if vf else None,
            sum(v + i for i, v in zip(rows_idx, vals["imix"]) if v is not None) if vi else None,
            len([v for v in vi if v > 0]), sum(v for v in vd if v > 0) and dec(sum(v for v in vd if v > 0), 6)]


AGG_SPECS = [Agg.count_rows(), Agg.count("imix"), Agg.sum("imix"), Agg.min("imix"), Agg.max("imix"), Agg.avg("imix"),
             Agg.sum("drev"), Agg.min("drev"), Agg.max("drev"), Agg.avg("drev"),
             Agg.count("fint"), Agg.sum("fint"), Agg.min("fint"), Agg.max("fint"), Agg.avg("fint"),
             Agg.sum(col("imix") + col("id")),                      # an operand of an aggregate's own expression
             Agg.count("id").where(P.gt("imix", V.Int64(0))),       # Agg.where on a computed column
             Agg.sum("drev").where(P.compare(col("drev"), ">", lit(0)))]


def test_aggregates_plain(big):
    got = big.builder(AGG_EXPRS).aggregate(AGG_SPECS)
    want = model_aggregates(big, list(range(big.n)))
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, AGG_SPECS[k], g, w)
    assert got[17] != 0


@pytest.mark.parametrize("key, limit", [("gk", None), ("gk", 1024), ("gd", None), ("gd", 1024)])
def test_aggregates_grouped_on_both_paths(big, key, limit):
    """GROUP BY a computed Int64 / Decimal key, every aggregate over computed arguments, on the hashed path (256 groups a stripe)
    and the wide one (max_groups above 256), the groups in first-appearance order"""
    keys, _ = M.eval_column(AGG_EXPRS[key], SCHEMA, big.rows)
    groups = {}
    for i, v in enumerate(keys):
        groups.setdefault(v, []).append(i)
    res = big.builder(AGG_EXPRS).aggregate(AGG_SPECS, group_by=[key], max_groups=limit)
    assert [k[0] for k, _ in res] == [None if v is None else v if key == "gk" else dec(v, 2) for v in groups], key
    for (k, got), idx in zip(res, groups.values()):
        want = model_aggregates(big, idx)
        for q, (g, w) in enumerate(zip(got, want)):
            if q == 17 and w == 0:
                w = None  # (no row of the group passes the condition: SUM over nothing is NULL)
            assert g == w, (key, limit, k, q, AGG_SPECS[q], g, w)


def test_float64_keys_stay_refused(big):
    with pytest.raises(capi.OrcGpuError) as e:  # as Float / Double keys are
        big.builder({"fsum": EXPRS["fsum"]}).aggregate([Agg.count_rows()], group_by=["fsum"])
    assert "fsum" in str(e.value)


def test_result_level_entry_point_on_a_hand_decoded_result():
    """orcgpu_result_compute_columns: columns appended to a result decoded through the C ABI, then read back, selected on and
    filtered like the result's own"""
    c = TA.ctx()
    n = 2 * 1000 + 65
    res, table = TA.stripe_result(n, 1000)
    ids, v = table.column("id").to_pylist(), table.column("v").to_pylist()
    schema = {"id": "int", "v": "int"}
    exprs = {"r": col("v") * col("id") + 3, "big": col("v") * (2 ** 62)}
    over = c.result_compute_columns(res, exprs, ["id", "v"])
    rows = [{"id": i, "v": x} for i, x in zip(ids, v)]
    want_r, over_r = M.eval_column(exprs["r"], schema, rows)
    want_b, over_b = M.eval_column(exprs["big"], schema, rows)
    assert over == over_r + over_b and over_b > 0 and over_r == 0

    def column(res, colm):
        out = []
        for b in range(res.n_batches):
            x = res.batch(b, colm)
            vals = np.frombuffer(x["values"], dtype=np.int64)[:x["length"]]
            valid = np.unpackbits(np.frombuffer(x["validity"], dtype=np.uint8), bitorder="little")[:x["length"]] if x["validity"] is not None else np.ones(x["length"], np.uint8)
            assert x["null_count"] == int((valid == 0).sum())
            out += [int(a) if p else None for a, p in zip(vals, valid)]
        return out

    assert column(res, 0) == ids and column(res, 1) == v       # the decode's own columns are where they were
    assert column(res, 2) == want_r and column(res, 3) == want_b
    # a second call, an unknown operand, a name of the result's: refused, the result unchanged
    for bad, code, words in (({"t": col("v") + 1}, 101, "already holds computed columns"),):
        with pytest.raises(capi.OrcGpuError) as e:
            c.result_compute_columns(res, bad, ["id", "v", "r", "big"])
        assert e.value.code == code and words in str(e.value)
    # the row filter on the computed column, by the result-level call
    kept = c.result_filter(res, P.gt("r", V.Int64(100)), ["id", "v", "r", "big"])
    exp = [i for i in range(n) if want_r[i] is not None and want_r[i] > 100]
    assert kept == len(exp) and column(res, 0) == exp and column(res, 2) == [want_r[i] for i in exp]
    res.free()
    res, _ = TA.stripe_result(65, 1000)
    for bad, code, words in (({"v": col("id") + 1}, 101, "'v' is the name of a root column"), ({"t": col("nope") + 1}, 101, "'nope'")):
        with pytest.raises(capi.OrcGpuError) as e:
            c.result_compute_columns(res, bad, ["id", "v"])
        assert e.value.code == code and words in str(e.value)
    res.select([(5, True), (20, False)])
    with pytest.raises(capi.OrcGpuError) as e:
        c.result_compute_columns(res, {"t": col("v") + 1}, ["id", "v"])
    assert e.value.code == 101 and "compute its columns first" in str(e.value)
    res.free()


def test_top_k_keys(big):
    names = ["isum", "drev"]
    full = concat_batches(list(big.builder([(k, EXPRS[k]) for k in names]).build()))
    for key, desc, nf in (("isum", False, False), ("isum", True, True), ("drev", True, False)):
        got = big.builder([(k, EXPRS[k]) for k in names]).top_k([SortKey(key, descending=desc, nulls_first=nf), SortKey("id")], 50)
        want, _ = TK.top_k_table(full, [(key, desc, nf), ("id", False, False)], 50)
        assert got.schema.names == want.schema.names and got.num_rows == 50
        for name in want.schema.names:
            assert got_values(got, name) == got_values(want, name), (key, desc, nf, name)


def test_device_output_equals_the_host_path(big):
    names = ["isum", "drev", "fsum"]
    host = concat_batches(list(big.builder([(k, EXPRS[k]) for k in names]).with_projection(["id", "a", "b", "p", "q", "x", "y"]).build()))
    reader = big.builder([(k, EXPRS[k]) for k in names]).with_projection(["id", "a", "b", "p", "q", "x", "y"]).with_device_output().build()
    dev = [b.to_pyarrow() for b in reader]
    assert reader.d2h_bytes() == 0
    table = concat_batches(dev)
    assert table.schema.names == host.schema.names
    for k in names:
        assert got_values(table, k) == got_values(host, k), k


def test_c_side_refusals(big, tmp_path):
    def refused(exprs, code, fragment, projection=None, path=None):
        b = ArrowReaderBuilder.try_new(path or big.path, ctx()).with_batch_size(BATCH).with_prefetch(0)
        if projection:
            b = b.with_projection(projection)
        with pytest.raises(capi.OrcGpuError) as e:
            list(b.with_computed_columns(exprs).build())
        assert e.value.code == code and fragment in str(e.value), str(e.value)

    refused({"a": col("b") + 1}, 101, "'a' is the name of a root column of the file")
    refused({"a": col("b") + 1}, 101, "'a' is the name of a root column of the file", projection=["b"])  # projected or not
    refused({"r": col("s") + 1}, 7, "column 's' cannot stand in the expression of computed column 'r'")
    refused({"r": col("nope") + 1}, 101, "column 'nope' in the expression of computed column 'r' is not a projected root column")
    refused({"r": col("a") + 1}, 101, "column 'a' in the expression of computed column 'r' is not a projected root column", projection=["b"])
    refused([("r", col("a") + 1), ("t", col("r") + 1)], 7, "computed column 't': its operand 'r' is a computed column")
    refused({"r": lit(1) + lit(2)}, 101, "computed column 'r': its expression holds no column")
    refused({"r": col("x") + col("a")}, 6, "computed column 'r' mixes the Float / Double column 'x'")
    e = col("q")
    for _ in range(9):
        e = e * col("q")
    refused({"r": e}, 7, "scale of more than 38")
    # a nested column in the projection beside computed columns
    nested = str(tmp_path / "nested.orc")
    orc.write_table(pa.table({"k": pa.array([1, 2, 3], pa.int64()), "st": pa.array([{"f": 1}, {"f": 2}, None], pa.struct([("f", pa.int64())]))}), nested)
    refused({"r": col("k") + 1}, 7, "the projected column 'st' is nested", path=nested)
    # set after the first batch
    b = ArrowReaderBuilder.try_new(big.path, ctx()).with_batch_size(BATCH).with_prefetch(0)
    assert b.stripe_count() == 4
    L = ctx().L
    handle = b._h
    assert L.orcgpu_reader_column_count(handle) == len(SCHEMA)  # (builds the reader)
    with pytest.raises(capi.OrcGpuError) as err:
        b.with_computed_columns({"r": col("a") + 1})
    assert err.value.code == 101 and "after the reader has been built" in str(err.value)


def test_without_computed_columns_nothing_changes(big):
    """a reader that is not given computed columns hands out what pyarrow reads of the file, and counts nothing"""
    reader = ArrowReaderBuilder.try_new(big.path, ctx()).with_batch_size(BATCH).with_prefetch(0).build()
    batches = list(reader)
    assert all(b.schema.names == big.names for b in batches)
    assert reader.computed_overflow_rows() == 0
    ours, theirs = concat_batches(batches), orc.ORCFile(big.path).read()
    for name in big.names:
        assert got_values(ours, name) == got_values(theirs, name), name
