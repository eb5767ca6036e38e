"""cast / round_ / floor / ceil / trunc on the GPU (orc_rust_amd.aggregate; the AX_TO_F64 .. AX_F64_ROUND ops of
device/agg_expr_eval.h's mixed interpreter inside compute_columns_conv_kernel, filter_expr_conv_kernel and the expression
aggregates' three *_conv_* kernels) against tests/conv_model.py: integers and Decimals exactly, a double bit for bit, a double sum
within tests/agg_model.py's float_bound of math.fsum, the tolerance tests/test_gpu_aggregate_expr.py uses.  Small files written with
pyarrow: 1, 63, 64, 65 and 257 rows in one stripe, 5000 rows in two, read in batches of 1024; Long, Decimal(18, 2), Decimal(38, 10),
Double, Float and Date columns with NULLs at word edges.  Every test but the last needs the new nodes."""
import decimal
import math

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import agg_expr_model as AEM
import agg_model as AM
import conv_model as M
import div_model as DM
import test_conv_model as TM
import test_gpu_div as D
from orc_rust_amd import capi
from orc_rust_amd import aggregate as A
from orc_rust_amd.aggregate import Agg, col
from orc_rust_amd.arrow_reader import ArrowReaderBuilder, concat_batches

pytestmark = pytest.mark.gpu

BATCH = 1024
SCHEMA = {"id": "int", "g": "int", "k": "int", "l": "int", "e": ("dec", 2), "w": ("dec", 10), "x": "float", "xf": "float", "f": "float", "d": "date", "dd": "float"}
ARROW = {"id": pa.int64(), "g": pa.int32(), "k": pa.int32(), "l": pa.int64(), "e": pa.decimal128(18, 2), "w": pa.decimal128(38, 10), "x": pa.float64(), "xf": pa.float64(),
         "f": pa.float32(), "d": pa.date32(), "dd": pa.float64()}
LONGS = [0, 1, -1, 2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, -(2 ** 53) - 1, 2 ** 63 - 1, -2 ** 63, 12345, -7, 10 ** 18]
DEC18 = [0, 5, -5, 50, -50, 149, 150, 151, -150, 250, -250, 10 ** 18 - 1, -(10 ** 18 - 1), 99, -99]
DEC38 = [0, 1, -1, 5 * 10 ** 9, -5 * 10 ** 9, 15 * 10 ** 9, 25 * 10 ** 9 - 1, 2 ** 53 + 1, 2 ** 64 + 1, -(2 ** 64) - 1, 10 ** 38 - 1, -(10 ** 38 - 1), 10 ** 37 + 5 * 10 ** 9,
         123456789012345678901234567890, 9223372036854775807 * 10 ** 10 + 9999999999, 9223372036854775808 * 10 ** 10]
DAYS = [0.0, 0.75, -0.25, 19000.5, -719468.0, 2932896.999, 2147483647.0, 2147483648.0, -2147483648.9, 1e12, float("nan"), -0.0]


def make_columns(n, seed=11):
    rng = np.random.default_rng(seed + n)

    def nulls(values, frac=0.12):
        out = [None if z else v for v, z in zip(values, rng.random(n) < frac)]
        for edge in (0, 63, 64, 127, 128, n - 1):
            if 0 <= edge < n and n > 1:
                out[edge] = None if edge % 2 == 0 else values[edge]
        return out

    def pick(pool, other):
        return [pool[int(v)] if c else o for v, c, o in zip(rng.integers(0, len(pool), n), rng.random(n) < 0.5, other)]

    c = {"id": list(range(n)), "g": nulls([int(v) for v in rng.integers(0, 5, n)], 0.1), "k": [int(v) for v in rng.integers(0, 400, n)]}
    c["l"] = nulls(pick(LONGS, [int(v) for v in rng.integers(-10 ** 9, 10 ** 9, n)]))
    c["e"] = nulls(pick(DEC18, [int(v) for v in rng.integers(-10 ** 16, 10 ** 16, n)]))
    c["w"] = nulls(pick(DEC38, [int(v) * 10 ** 7 + 5 for v in rng.integers(-10 ** 15, 10 ** 15, n)]))
    c["x"] = nulls(pick(TM.DOUBLES, [float(v) for v in rng.uniform(-1e6, 1e6, n)]))
    c["xf"] = nulls([float(v) for v in rng.uniform(-1e6, 1e6, n)])
    c["f"] = nulls(pick(D.FLOATS, [float(np.float32(v)) for v in rng.uniform(-100, 100, n)]))
    c["d"] = nulls([int(v) for v in rng.integers(-800000, 3000000, n)])
    c["dd"] = nulls(pick(DAYS, [float(v) + 0.5 for v in rng.integers(-800000, 3000000, n)]))
    return c


def arrow_table(c, names):
    arrays = []
    for name in names:
        t = ARROW[name]
        if pa.types.is_decimal(t):
            arrays.append(pa.array([None if v is None else decimal.Decimal(v).scaleb(-t.scale, D.EXACT) for v in c[name]], t))
        elif t == pa.date32():
            arrays.append(pa.array(c[name], pa.int32()).cast(pa.date32()))
        else:
            arrays.append(pa.array(c[name], t))
    return pa.table(arrays, names=names)


class File:
    def __init__(self, tmpdir, n, stripes=1):
        self.n, self.names = n, list(SCHEMA)
        self.c = make_columns(n)
        self.rows = [{k: self.c[k][i] for k in self.names} for i in range(n)]
        self.path = str(tmpdir / ("conv%d.orc" % n))
        if stripes == 1:
            orc.write_table(arrow_table(self.c, self.names), self.path, compression="uncompressed", stripe_size=64 << 20)
        else:  # a stripe ends where the writer next looks at its size: after a batch of 4096 rows
            orc.write_table(arrow_table(self.c, self.names), self.path, compression="uncompressed", stripe_size=1024, batch_size=4096)
        assert orc.ORCFile(self.path).nstripes == stripes

    def builder(self, exprs=None):
        b = ArrowReaderBuilder.try_new(self.path, D.ctx()).with_batch_size(BATCH)
        return b.with_computed_columns(exprs) if exprs else b

    def model(self, e):
        vals, over = M.computed_column(e, SCHEMA, self.rows)
        if M.computed_type(e, SCHEMA)[0] == "float64":
            vals = [None if v is None else D.bits(v) for v in vals]
        return vals, over


def exprs():
    from orc_rust_amd.aggregate import cast, ceil, coalesce, decimal_, floor, round_, trunc, when, year
    l, e, w, x, f, dd = (col(n) for n in ("l", "e", "w", "x", "f", "dd"))
    return {
        # every conversion on its own
        "l_f": cast(l, "float64"), "e_f": cast(e, "float64"), "w_f": cast(w, "float64"),            # both paths of to-double
        "x_d2": cast(x, decimal_(2)), "x_d38": cast(x, decimal_(38)), "f_d0": cast(f, decimal_(0)),  # a double's exact value, NaN / inf / 1e38 overflow
        "e_d10": cast(e, decimal_(10)), "w_d2": cast(w, decimal_(2)), "l_d38": cast(l, decimal_(38)),  # up (checked), down (half away), up past 128 bits
        "l_i": cast(l * l, "int64"), "w_i": cast(w, "int64"), "x_i": cast(x, "int64"),                # the value, truncated, truncated; outside int64
        "w_r4": round_(w, 4), "e_r0": round_(e), "l_r": round_(l, 3), "x_r": round_(x),
        "w_fl": floor(w), "w_ce": ceil(w), "w_tr": trunc(w), "x_fl": floor(x), "x_ce": ceil(x), "x_tr": trunc(f),
        # the mixed programs
        "m1": cast(e, "float64") * x,
        "m2": cast(x * 100, decimal_(2)) + e,
        "m3": when(x > 0, cast(x, "int64"), floor(e)),            # the untaken branch overflows (NaN to int64) and counts nothing
        "m4": year(cast(dd, "int64")),
        "m5": cast(l, "float64") / 3,
        "m6": floor(w) % 7 + year(floor(cast(dd, decimal_(1)))),   # integers of scale 0 below // % and a date part
        "m7": coalesce(cast(cast(x, decimal_(4)), "float64"), cast(l, "float64"), 0.5),
        "m8": cast(floor(e / 1000), "int64"),
        # a Date column is int64 days wherever a computed column reads it: below a conversion below a date part too
        "d1": year(cast("d", "int64")) * 100 + cast(cast("d", "float64") / 7, "int64") % 53,
    }


def parts(ex, most=8):
    items = list(ex.items())
    return [dict(items[k:k + most]) for k in range(0, len(items), most)]


def arrow_type_of(e):
    kind, s = M.computed_type(e, SCHEMA)
    return pa.int64() if kind == "int64" else pa.float64() if kind == "float64" else pa.decimal128(38, s)


def check_columns(f, table, reader, ex):
    over = 0
    for k, e in ex.items():
        want, o = f.model(e)
        over += o
        assert table.schema.field(k).type == arrow_type_of(e), k
        got = D.got_values(table, k)
        assert got == want, (k, [(n, a, b, f.rows[n]) for n, (a, b) in enumerate(zip(got, want)) if a != b][:3])
    assert reader.computed_overflow_rows() == over
    return over


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    return File(tmp_path_factory.mktemp("conv"), 5000, stripes=2)


def test_the_nodes_are_new():
    """Fails without the feature: the names do not exist at the parent commit, and the C nodes 30 .. 34 are unknown nodes there."""
    from orc_rust_amd.aggregate import EXPR_CAST, EXPR_TRUNC, cast, ceil, decimal_, floor, round_, trunc  # noqa: F401
    assert (EXPR_CAST, EXPR_TRUNC) == (30, 34)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_rows_against_the_model(tmp_path, n):
    f = File(tmp_path, n)
    for ex in parts(exprs()):
        reader = f.builder(ex).build()
        batches = list(reader)
        for b in batches:
            b.validate(full=True)
        table = concat_batches(batches)
        assert table.num_rows == n and table.schema.names == f.names + list(ex)
        check_columns(f, table, reader, ex)


def test_two_stripes_host_and_device_output(big):
    over = 0
    for ex in parts(exprs()):
        reader = big.builder(ex).build()
        host = concat_batches(list(reader))
        over += check_columns(big, host, reader, ex)
        reader = big.builder(ex).with_device_output().build()
        dev = concat_batches([b.to_pyarrow() for b in reader])
        assert reader.d2h_bytes() == 0
        check_columns(big, dev, reader, ex)
    assert over > 0
    # the data holds what the test is about, by the model's per-row outcomes
    ex = exprs()
    m3 = [M.computed_value(ex["m3"], SCHEMA, r) for r in big.rows]
    nan_rows = [o for r, o in zip(big.rows, m3) if r["x"] is not None and r["x"] != r["x"] and r["e"] is not None]
    assert nan_rows and all(o[1] is False and o[0] is not None for o in nan_rows)       # NaN > 0 is FALSE: the cast is not taken, nothing counts
    assert (None, True) in m3                                                              # 1e38 > 0: the cast is taken and overflows
    assert (None, True) in [M.computed_value(ex["m4"], SCHEMA, r) for r in big.rows]       # days past int32
    for k in ("x_d2", "x_i", "w_i", "l_d38", "l_i"):
        assert big.model(ex[k])[1] > 0, k
    for k in ("l_f", "e_f", "w_f", "w_r4", "w_fl", "x_fl", "x_r"):
        assert big.model(ex[k])[1] == 0, k
    assert arrow_type_of(ex["m2"]) == pa.decimal128(38, 2) and arrow_type_of(ex["m3"]) == pa.decimal128(38, 0) and arrow_type_of(ex["m6"]) == pa.decimal128(38, 0) and arrow_type_of(ex["m4"]) == pa.int64() and arrow_type_of(ex["m8"]) == pa.int64()
    # cast(l, 'float64') / 3 is one IEEE division of the nearest double; l / 3 is a Decimal at scale 6
    vals = D.got_values(concat_batches(list(big.builder({"q": col("l") / 3}).build())), "q")
    assert vals == DM.computed_column(col("l") / 3, SCHEMA, big.rows)[0] and arrow_type_of(col("l") / 3) == pa.decimal128(38, 6)


def test_filter_leaves_count_their_overflows(big):
    from orc_rust_amd.aggregate import cast, ceil, decimal_, floor, round_, trunc, year
    cases = [(ceil("w"), ">", trunc("w"), False), (cast(col("l") * col("l"), "int64"), ">", 10 ** 6, True), (floor("x"), "<=", col("xf"), False),
             (cast(cast("x", "int64"), "float64"), "<", col("xf"), True),  # a side of doubles that overflows inside: counted
             (round_("x") + trunc("f"), ">", ceil("xf"), False), (year(cast("d", "int64")) + cast(cast("d", "float64") / 7, "int64"), ">", 2000, False),
             (cast("e", "float64") * col("x"), ">", 1.5, False), (cast("x", "int64"), "<", col("l"), True), (floor("w"), ">=", cast("xf", decimal_(3)), False),
             (cast("x", decimal_(2)), "<=", col("e"), True), (round_("w", 2), "=", cast("w", decimal_(2)), False), (cast(col("l"), "float64") / 3, "<", col("xf"), False)]
    for lhs, op, rhs, overflows in cases:
        keep, over = [], 0
        for i, r in enumerate(big.rows):
            t, o = M.filter_leaf(lhs, op, rhs, r, SCHEMA)
            over += 1 if o else 0
            if t is True:
                keep.append(i)
        assert keep and (over > 0) == overflows, (lhs, op, rhs)
        for prune in (True, False):
            reader = big.builder().with_row_filter(D.P.compare(lhs, op, rhs), prune=prune).with_row_group_pruning(prune).build()
            batches = list(reader)
            got = concat_batches(batches).column("id").to_pylist() if batches else []
            assert got == keep, (lhs, op, rhs, prune)
            assert reader.filter_overflow_rows() == over, (lhs, op, rhs, prune)


def specs():
    """every conversion through the aggregates' kernels: the casts, ROUND / FLOOR / CEIL / TRUNC of a Decimal (AX_RESCALE) and of a
    double (AX_F64_ROUND), AX_FIT_I64, and the untaken branch that overflows -- over `x`, which holds NaN, the infinities and 1e38"""
    from orc_rust_amd.aggregate import cast, ceil, decimal_, floor, round_, trunc, when
    x, xf, e = col("x"), col("xf"), col("e")
    return [Agg.sum(cast(e, "float64") * xf), Agg.sum(cast(xf * 100, decimal_(2)) + e), Agg.avg(cast(floor(e), "int64")),
            Agg.sum(when(xf > 0, cast(xf, "int64"), floor(e))), Agg.avg(cast("w", "float64")), Agg.avg(cast(xf, decimal_(3))),
            Agg.sum(round_(e, 1)), Agg.sum(ceil(e) - trunc(e)), Agg.avg(trunc(e)), Agg.sum(round_(e)),
            Agg.sum(round_(xf) + floor(xf)), Agg.avg(ceil(xf) - trunc(xf)), Agg.sum(trunc(xf * 0.5)),
            Agg.sum(cast(col("g") * col("k"), "int64")),
            Agg.sum(when((x > 0) & (x < 1e18), cast(x, "int64"), floor(e)))]


def check_aggs(big, idx, got, what):
    rows = [big.rows[i] for i in idx]
    assert len(got) == len(specs())
    for n, (spec, g) in enumerate(zip(specs(), got)):
        kind, scale = M.computed_type(spec.expr, SCHEMA)
        vals = [v for v in (M.agg_row(spec.expr, SCHEMA, r) for r in rows) if v is not None]
        assert AEM.ROW_OVERFLOW not in vals, (what, n)
        avg = spec.op == A.AVG_EXPR
        if not vals:
            assert g is None, (what, n)
        elif kind == "float64":  # a double sum: any order of the reduction, within the textbook bound
            want = math.fsum(vals) / (len(vals) if avg else 1)
            bound = AM.float_bound(vals) / (len(vals) if avg else 1)
            assert isinstance(g, float) and abs(g - want) <= bound, (what, n, g, want, bound)
        elif kind == "int64":
            assert g == (AEM.avg_int(sum(vals), len(vals)) if avg else sum(vals)), (what, n)
        else:
            assert g == (D.dec(*AEM.avg_decimal(sum(vals), len(vals), scale)) if avg else D.dec(sum(vals), scale)), (what, n)


def test_aggregates_plain_narrow_and_wide(big):
    from orc_rust_amd.aggregate import cast, decimal_, floor
    got = big.builder().aggregate(specs())
    assert None not in got
    last = specs()[-1].expr  # the data holds the untaken overflow: NaN, an infinity or 1e38 beside a Decimal that is there
    assert any(r["x"] is not None and r["e"] is not None and (r["x"] != r["x"] or r["x"] >= 1e38) and M.agg_row(last, SCHEMA, r) not in (None, AEM.ROW_OVERFLOW)
               for r in big.rows)
    check_aggs(big, range(big.n), got, "plain")
    # the same call again: a double sum is the same bits on every run
    assert [v.hex() if isinstance(v, float) else v for v in big.builder().aggregate(specs())] == [v.hex() if isinstance(v, float) else v for v in got]
    for key, limit in (("g", None), ("k", 512)):  # 6 groups on the narrow path, 400 under max_groups = 512 on the wide one
        groups = {}
        for i, r in enumerate(big.rows):
            groups.setdefault(r[key], []).append(i)
        res = big.builder().aggregate(specs(), group_by=[key], max_groups=limit)
        assert [k[0] for k, _ in res] == list(groups)
        for (k, vals), idx in zip(res, groups.values()):
            check_aggs(big, idx, vals, (key, k))
    # GROUP BY a computed bucket that needs a conversion to be an integer
    bucket = cast(floor(col("e") / 10 ** 14), "int64")
    want = big.model(bucket)[0]
    groups = {}
    for i in range(big.n):
        groups.setdefault(want[i], []).append(i)
    res = big.builder({"b": bucket}).aggregate([Agg.count_rows(), Agg.sum(cast("b", decimal_(1)))], group_by=["b"])
    assert [k[0] for k, _ in res] == list(groups)
    for (k, vals), idx in zip(res, groups.values()):
        assert vals == [len(idx), None if k[0] is None else D.dec(k[0] * 10 * len(idx), 1)], k
    # an overflow inside an expression of doubles is AGG_OVERFLOW too; so is one in the INT class, on each path
    for spec in (Agg.sum(cast(cast("x", "int64"), "float64")), Agg.sum(cast("x", decimal_(2)))):
        for kw in ({}, {"group_by": ["g"]}, {"group_by": ["k"], "max_groups": 512}):
            with pytest.raises(OverflowError):
                big.builder().aggregate([spec], **kw)


def test_c_side_refusals(big):
    from orc_rust_amd.aggregate import EXPR_CAST, EXPR_ROUND, Expr, cast, floor, round_, year

    def refused(run, code, *fragments):
        with pytest.raises(capi.OrcGpuError) as e:
            run()
        assert e.value.code == code and all(f in str(e.value) for f in fragments), str(e.value)
    refused(lambda: list(big.builder({"r": col("e") * col("x")}).build()), 6, "mixes the Float / Double column 'x'", "cast")
    refused(lambda: list(big.builder({"r": cast("e", "float64") + col("e")}).build()), 6, "Float / Double", "cast")
    refused(lambda: big.builder().aggregate([Agg.sum(round_("x", 2))]), 7, "ROUND", "decimal")
    refused(lambda: list(big.builder().with_row_filter(year(floor("x")) > 2000, prune=False).build()), 6, "row filter:", "year()")
    # in an aggregate a Date column is days only DIRECTLY below a date part: what stands below a conversion is not "below the part"
    assert big.builder().aggregate([Agg.sum(year("d"))])[0] is not None
    refused(lambda: big.builder().aggregate([Agg.sum(year(cast("d", "int64")))]), 6, "column 'd'")
    refused(lambda: list(big.builder({"r": Expr(EXPR_CAST, (col("l"),), value_type=5)}).build()), 101, "CAST", "target")
    refused(lambda: list(big.builder({"r": Expr(EXPR_CAST, (col("l"),), value_type=8, scale=39)}).build()), 101, "CAST", "scale")
    refused(lambda: list(big.builder({"r": Expr(EXPR_ROUND, (col("l"),), scale=-1)}).build()), 101, "ROUND", "digits")
    refused(lambda: list(big.builder({"r": Expr(EXPR_ROUND, (), scale=0)}).build()), 101, "ROUND", "without its child")


def test_a_program_without_a_new_node_gives_what_it_gave(big):
    """the instantiations without the conversions still run their programs: the answers of the existing models"""
    from orc_rust_amd.aggregate import when
    import cond_model as CDM
    ex = {"s": col("e") * 2 + col("w"), "q": col("e") / col("l"), "c": when(col("l") > 0, col("e"), -col("e")), "fx": col("x") * 2.0 - col("xf")}
    reader = big.builder(ex).build()
    table = concat_batches(list(reader))
    over = 0
    for k, e in ex.items():
        vals, o = CDM.computed_column(e, SCHEMA, big.rows)
        if CDM.computed_type(e, SCHEMA)[0] == "float64":
            vals = [None if v is None else D.bits(v) for v in vals]
        over += o
        assert D.got_values(table, k) == vals, k
    assert reader.computed_overflow_rows() == over
    want = [i for i in range(big.n) if DM.filter_leaf(col("l") % 1000, "<", col("g") * 300, big.rows[i], SCHEMA)[0] is True]
    assert concat_batches(list(big.builder().with_row_filter(col("l") % 1000 < col("g") * 300, prune=False).build())).column("id").to_pylist() == want
    vals = [v for v in (CDM.agg_row(col("e") * col("l"), SCHEMA, r) for r in big.rows) if v is not None]
    assert big.builder().aggregate([Agg.sum(col("e") * col("l"))]) == [D.dec(sum(vals), 2)]
