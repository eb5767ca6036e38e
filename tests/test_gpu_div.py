"""a / b, a // b, a % b and divide() on the GPU (orc_rust_amd.aggregate; the AX_DIV / AX_FLOOR_DIV / AX_MOD / AX_SWAP ops of
device/agg_expr_eval.h inside compute_columns_div_kernel, filter_expr_div_kernel and the expression aggregates' *_div_* kernels)
against tests/div_model.py, row for row and exactly; doubles bit for bit against numpy.  Files are written in the test with
pyarrow, one stripe or four, a few thousand rows at most.  Every test here needs the new operators: none passes without the feature."""
import decimal
import struct

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import agg_expr_model as AEM
import div_model as M
import selection_model as SM
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg, col, divide, year
from orc_rust_amd.arrow_reader import ArrowReaderBuilder, concat_batches
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
from orc_rust_amd.top_k import SortKey

pytestmark = pytest.mark.gpu

BATCH = 1024
EXACT = decimal.Context(prec=80)
SCHEMA = {"id": "int", "g": "int", "t": "int", "h": "int", "i": "int", "L": "int", "M": "int", "d": "date", "dn": "date", "p": ("dec", 2), "q": ("dec", 4),
          "ps": ("dec", 2), "kn": "int", "f": "float", "x": "float", "y": "float"}
ARROW = {"id": pa.int64(), "g": pa.int32(), "t": pa.int8(), "h": pa.int16(), "i": pa.int32(), "L": pa.int64(), "M": pa.int64(), "d": pa.date32(), "dn": pa.date32(),
         "p": pa.decimal128(38, 2), "q": pa.decimal128(38, 4), "ps": pa.decimal128(12, 2), "kn": pa.int32(), "f": pa.float32(), "x": pa.float64(), "y": pa.float64()}
# magnitudes on either side of 2^32, 2^64 and 2^96, +-1, 0, 38-digit values: every path of the divide, and the overflows
LONGS = [0, 1, -1, 2, -2, 3, 5, -5, 7, -7, 16, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, -2 ** 32 - 1, 2 ** 62, 2 ** 63 - 1, -2 ** 63, -2 ** 63 + 1]
WIDE = [0, 1, -1, 3, 250, -250, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1, 2 ** 64, 2 ** 64 + 1, -2 ** 64 - 1, 2 ** 70 + 5, 2 ** 95, 2 ** 96 - 1, 2 ** 96, -2 ** 96 - 1, 2 ** 100 + 1, 10 ** 37,
        10 ** 38 - 1, -(10 ** 38 - 1)]
NAN = struct.unpack("<d", struct.pack("<Q", 0x7ff8000000000000))[0]  # ONE NaN: which operand's payload a quotient of two NaNs keeps is not IEEE's to say
DOUBLES = [0.0, -0.0, 1.0, -1.0, 3.0, 0.1, 1e308, -1e308, 5e-324, 1e-308, float("inf"), float("-inf"), NAN, 2.0 ** 53 + 2, 1.5]
FLOATS = [0.0, -0.0, 1.0, -3.0, 0.5, 2.0 ** 100, float("inf"), 1.25, -7.0]  # (exact in a Float32)
EXPRS_A = {
    "pq": col("p") / col("q"),                          # Decimal by Decimal: scale 6, the dividend times 10^8; every path of the divide
    "pL": col("p") / col("L"),                          # Decimal by Long: the dividend times 10^4
    "LM": col("L") / col("M"),                          # int / int is a Decimal at scale 6
    "LM0": divide("L", "M", scale=0),                   # exact halves of both signs: away from zero
    "fl": col("L") // col("M"), "md": col("L") % col("M"),  # the floor rule, negative operands, -2^63 // -1 past Int64
    "qp2": divide(col("q") - col("p"), col("p") + 1, scale=2),  # operands that are expressions; q - p aligns the scales first
    "rev": col("i") % (col("h") + col("t")),            # the right child goes first: AX_SWAP
}
EXPRS_B = {
    "b16": col("id") % 16, "wk": col("d") // 7,         # a bucket, a week number
    "th": col("t") // col("h") + col("i") % col("h"),   # Byte, Short, Int
    "ym": year("d") % 100 * col("ps"),                  # an integer subtree of scale 0 inside a Decimal expression
    "xy": col("x") / col("y"), "fx": col("f") / col("x"), "x3": 1.0 / (col("x") * 3.0),  # doubles (a Float widened first): IEEE, NaN and the infinities
    "pw": divide(col("p") * col("ps"), col("q"), scale=0),  # a product first: a dividend that leaves 128 bits before the power of ten
}
_CTX = None


def ctx():
    global _CTX
    if _CTX is None:
        _CTX = capi.Context()
    return _CTX


def make_columns(n, seed=5):
    """name -> the model's values (ints, a Decimal's unscaled int, floats; None: NULL).  NULLs at word edges; dn and id have none."""
    rng = np.random.default_rng(seed + n)

    def nulls(values, frac=0.12):
        out = [None if z else v for v, z in zip(values, rng.random(n) < frac)]
        for edge in (0, 63, 64, 127, 128, n - 1):
            if 0 <= edge < n:
                out[edge] = None if edge % 2 == 0 else values[edge]
        return out

    def pick(pool):
        return [pool[int(v)] for v in rng.integers(0, len(pool), n)]

    c = {"id": list(range(n)), "g": nulls([int(v) for v in rng.integers(0, 5, n)], 0.1)}
    c["t"] = nulls([int(v) for v in rng.integers(-128, 128, n)])
    c["h"] = nulls([int(v) if k % 9 else 0 for k, v in enumerate(rng.integers(-300, 300, n))])  # zero divisors
    c["i"] = nulls([int(v) for v in rng.integers(-2 ** 31, 2 ** 31, n)])
    c["L"], c["M"] = nulls(pick(LONGS)), nulls(pick(LONGS))
    c["d"] = nulls([int(v) for v in rng.integers(-800000, 3000000, n)])
    c["dn"] = [int(v) for v in rng.integers(8000, 11000, n)]
    c["p"], c["q"] = nulls(pick(WIDE)), nulls(pick(WIDE))
    c["ps"] = nulls([int(v) for v in rng.integers(-10 ** 6, 10 ** 6, n)], 0.1)
    c["kn"] = nulls([int(v) for v in rng.integers(1, 50, n)], 0.1)  # never zero: what the aggregates divide by
    c["f"], c["x"], c["y"] = nulls(pick(FLOATS)), nulls(pick(DOUBLES)), nulls(pick(DOUBLES))
    for row, (a, b) in enumerate(((5, 2), (-5, 2), (5, -2), (-2 ** 63, -1), (7, 0), (0, 0), (-7, 2), (7, -2))):  # halves, the extremes, zero divisors
        if 2 * row + 1 < n:
            c["L"][2 * row + 1], c["M"][2 * row + 1] = a, b
    return c


def arrow_table(c, names):
    arrays = []
    for name in names:
        t = ARROW[name]
        if pa.types.is_decimal(t):
            arrays.append(pa.array([None if v is None else decimal.Decimal(v).scaleb(-t.scale, EXACT) for v in c[name]], t))
        elif t == pa.date32():
            arrays.append(pa.array(c[name], pa.int32()).cast(pa.date32()))
        else:
            arrays.append(pa.array(c[name], t))
    return pa.table(arrays, names=names)


class File:
    def __init__(self, tmpdir, n, stripes=1, tag="f"):
        self.n, self.names = n, list(SCHEMA)
        self.c = make_columns(n)
        self.rows = [{k: self.c[k][i] for k in self.names} for i in range(n)]
        self.path = str(tmpdir / ("%s%d.orc" % (tag, n)))
        orc.write_table(arrow_table(self.c, self.names), self.path, compression="uncompressed", row_index_stride=1000, stripe_size=(64 << 20) if stripes == 1 else 1024)
        assert orc.ORCFile(self.path).nstripes == (1 if stripes == 1 else (n + 1023) // 1024)

    def builder(self, exprs=None, prefetch=0):
        b = ArrowReaderBuilder.try_new(self.path, ctx()).with_batch_size(BATCH).with_prefetch(prefetch)
        return b.with_computed_columns(exprs) if exprs else b

    def model(self, e):
        """the column as got_values spells it, and the overflow count"""
        vals, over = M.computed_column(e, SCHEMA, self.rows)
        if M.computed_type(e, SCHEMA)[0] == "float64":
            vals = [None if v is None else bits(v) for v in vals]
        return vals, over


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def arrow_type_of(e):
    kind, s = M.computed_type(e, SCHEMA)
    return pa.int64() if kind == "int64" else pa.float64() if kind == "float64" else pa.decimal128(38, s)


def got_values(table, name):
    """the column as the model spells it: ints, a Decimal's unscaled int, a double's bits"""
    t = table.column(name).type
    if pa.types.is_date(t):
        return table.column(name).cast(pa.int32()).to_pylist()
    vals = table.column(name).to_pylist()
    if pa.types.is_decimal(t):
        return [None if v is None else int(v.scaleb(t.scale, EXACT)) for v in vals]
    if pa.types.is_floating(t):
        return [None if v is None else bits(v) for v in vals]
    return vals


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    return File(tmp_path_factory.mktemp("div"), 3 * 1024 + 1, stripes=4, tag="big")  # four stripes, the last of ONE row


def check_columns(f, table, reader, exprs):
    over = 0
    for k, e in exprs.items():
        want, o = f.model(e)
        over += o
        assert table.schema.field(k).type == arrow_type_of(e) and table.schema.field(k).nullable, k
        assert got_values(table, k) == want, k
    assert reader.computed_overflow_rows() == over
    return over


@pytest.mark.parametrize("n, stripes", [(1, 1), (63, 1), (64, 1), (65, 1), (1024, 1), (1025, 1), (2049, 1), (3073, 4)])
def test_rows_against_the_model(tmp_path, n, stripes):
    f = File(tmp_path, n, stripes=stripes)
    for exprs in (EXPRS_A, EXPRS_B):
        reader = f.builder(list(exprs.items())).build()
        batches = list(reader)
        for b in batches:
            b.validate(full=True)
        table = concat_batches(batches)
        assert table.num_rows == n and table.schema.names == f.names + list(exprs) and got_values(table, "L") == f.c["L"]
        over = check_columns(f, table, reader, exprs)
        assert n < 64 or over > 0  # zero divisors, products that leave 128 bits, -2^63 // -1
    assert arrow_type_of(EXPRS_A["LM"]) == pa.decimal128(38, 6) and arrow_type_of(EXPRS_A["fl"]) == pa.int64() and arrow_type_of(EXPRS_B["xy"]) == pa.float64()
    if n >= 1024:  # every path of the divide runs: by the magnitudes of pq's dividend (p * 10^8) and divisor
        paths = {(abs(r["p"] * 10 ** 8) >= 2 ** 64, abs(r["q"]) >= 2 ** 64) for r in f.rows if r["p"] is not None and r["q"] and M.fits(r["p"] * 10 ** 8)}
        assert paths == {(False, False), (True, False), (True, True), (False, True)}
        lm0 = dict(zip(zip(f.c["L"], f.c["M"]), M.computed_column(EXPRS_A["LM0"], SCHEMA, f.rows)[0]))
        assert (lm0[(5, 2)], lm0[(-5, 2)], lm0[(5, -2)], lm0[(7, 0)], lm0[(-2 ** 63, -1)]) == (3, -3, -3, None, 2 ** 63)


def test_doubles_are_numpys_bit_for_bit(big):
    table = concat_batches(list(big.builder({"xy": EXPRS_B["xy"], "fx": EXPRS_B["fx"]}).with_projection(["f", "x", "y"]).build()))
    for name, a, b in (("xy", "x", "y"), ("fx", "f", "x")):
        rows = [k for k in range(big.n) if big.c[a][k] is not None and big.c[b][k] is not None]
        with np.errstate(all="ignore"):
            want = np.array([big.c[a][k] for k in rows], dtype=np.float64) / np.array([big.c[b][k] for k in rows], dtype=np.float64)
        got = got_values(table, name)
        assert [got[k] for k in rows] == [bits(v) for v in want.tolist()], name
        assert all(got[k] is None for k in range(big.n) if k not in set(rows))
        assert any(v != v for v in want.tolist()) and any(v == float("inf") for v in want.tolist()) and any(v == float("-inf") for v in want.tolist())


def test_no_present_stream_and_the_device_output_path(big):
    exprs = {"wk": col("dn") // 7, "wd": col("dn") % 7, "r": col("dn") / (col("id") + 1)}
    host = concat_batches(list(big.builder(exprs).with_projection(["id", "dn"]).build()))
    for k, e in exprs.items():
        want, over = big.model(e)
        assert got_values(host, k) == want and None not in want and over == 0, k
    reader = big.builder(EXPRS_A).with_projection(["t", "h", "i", "L", "M", "p", "q"]).with_device_output().build()
    dev = concat_batches([b.to_pyarrow() for b in reader])
    assert reader.d2h_bytes() == 0
    assert check_columns(big, dev, reader, EXPRS_A) > 0


def test_poison_and_read_ahead(big, monkeypatch):
    monkeypatch.setenv("ORCGPU_POISON", "0xA5")  # a value or validity word left unwritten shows
    for prefetch in (0, 2):
        table = concat_batches(list(big.builder(EXPRS_A, prefetch=prefetch).build()))
        for k, e in EXPRS_A.items():
            assert got_values(table, k) == big.model(e)[0], (k, prefetch)


def kept_by(big, lhs, op, rhs, among):
    keep, over = [], 0
    for i in among:
        t, o = M.filter_leaf(lhs, op, rhs, big.rows[i], SCHEMA)
        over += 1 if o else 0
        if t is True:
            keep.append(i)
    return keep, over


def test_filter_leaves_under_a_selection_with_pruning_on_and_off(big):
    sel = [(100, False), (30, True), (900, False), (70, True), (1200, False), (500, True), (273, False)]  # (rows, skip), to the file's end
    assert sum(count for count, _ in sel) == big.n
    stripe_rows = [1024, 1024, 1024, 1]
    picked = [1024 * s + i for s, ranges in enumerate(SM.file_batches(sel, stripe_rows, BATCH)) for start, length in ranges for i in range(start, start + length)]
    # (lhs, op, rhs, whether the leaf overflows on some rows)
    cases = [(col("id") % 16, "=", 3, False), (col("L") // col("M"), "<", col("i") % 1000, True), (col("p") / col("q"), ">=", decimal.Decimal("0.5"), True),
             (col("ps") / col("kn"), "<", col("ps"), False), (col("x") / col("y"), ">", 0.0, False), (col("i"), ">", col("i") // col("h") * col("h"), True)]
    for lhs, op, rhs, overflows in cases:
        pred = P.compare(lhs, op, rhs)
        for use_sel in (False, True):
            among = picked if use_sel else list(range(big.n))
            want, over = kept_by(big, lhs, op, rhs, among)
            assert want, pred
            for prune in (True, False):
                b = big.builder().with_row_filter(pred, prune=prune).with_row_group_pruning(prune)
                if use_sel:
                    b = b.with_row_selection(sel)
                reader = b.build()
                batches = list(reader)
                got = concat_batches(batches).column("id").to_pylist() if batches else []
                assert got == want, (pred, use_sel, prune)
                assert reader.filter_overflow_rows() == over, (pred, use_sel, prune)
            assert (over > 0) == overflows, (pred, use_sel)
    # NOT over a leaf: UNKNOWN (a NULL, a zero divisor) stays out on both sides
    t = concat_batches(list(big.builder().with_row_filter(P.not_((col("L") % col("M")).eq(0)), prune=False).build()))
    assert t.column("id").to_pylist() == kept_by(big, col("L") % col("M"), "!=", 0, range(big.n))[0]


def dec(total, scale):
    return decimal.Decimal(total).scaleb(-scale, EXACT)


def model_aggs(big, idx):
    """SUM(ps / kn), AVG(ps / kn), COUNT(*) WHERE id % 16 = 3, SUM(i // kn), AVG(id % 7) over the rows idx"""
    unit = [v for v in (M.agg_row(col("ps") / col("kn"), SCHEMA, big.rows[i]) for i in idx) if v is not None]
    fl = [v for v in (M.agg_row(col("i") // col("kn"), SCHEMA, big.rows[i]) for i in idx) if v is not None]
    wd = [v for v in (M.agg_row(col("id") % 7, SCHEMA, big.rows[i]) for i in idx) if v is not None]
    avg = AEM.avg_decimal(sum(unit), len(unit), 6) if unit else None
    return [dec(sum(unit), 6) if unit else None, dec(*avg) if avg else None, sum(1 for i in idx if i % 16 == 3), sum(fl) if fl else None, AEM.avg_int(sum(wd), len(wd)) if wd else None]


SPECS = [Agg.sum(col("ps") / col("kn")), Agg.avg(col("ps") / col("kn")), Agg.count_rows().where((col("id") % 16).eq(3)), Agg.sum(col("i") // col("kn")), Agg.avg(col("id") % 7)]


def test_aggregates_plain_and_grouped(big):
    got = big.builder().aggregate(SPECS)
    assert got == model_aggs(big, range(big.n)) and got[2] > 0 and got[0] is not None
    groups = {}
    for i, r in enumerate(big.rows):
        groups.setdefault(r["g"], []).append(i)
    for limit in (None, 1024):
        res = big.builder().aggregate(SPECS, group_by=["g"], max_groups=limit)
        assert [k[0] for k, _ in res] == list(groups)
        for (k, vals), idx in zip(res, groups.values()):
            assert vals == model_aggs(big, idx), (limit, k)
    # a zero divisor, a product that leaves 128 bits: AGG_OVERFLOW, as any operation that leaves 128 bits is
    assert any(M.agg_row(col("L") / col("M"), SCHEMA, r) == AEM.ROW_OVERFLOW for r in big.rows)
    for e in (col("L") / col("M"), col("t") % col("h"), col("p") / col("q")):
        with pytest.raises(OverflowError):
            big.builder().aggregate([Agg.sum(e)])
    with pytest.raises(OverflowError):
        big.builder().aggregate([Agg.avg(col("i") // col("h"))], group_by=["g"], max_groups=1024)


@pytest.mark.parametrize("limit", [None, 1024])
def test_group_by_a_computed_bucket_on_both_paths(big, limit):
    exprs = {"b16": col("id") * 7 % 16, "wk": col("dn") // 7 % 3}
    vals = {k: big.model(e)[0] for k, e in exprs.items()}
    for keys in (["b16"], ["b16", "wk"]):
        groups = {}
        for i in range(big.n):
            groups.setdefault(tuple(vals[k][i] for k in keys), []).append(i)
        assert len(groups) == (16 if len(keys) == 1 else 48)
        res = big.builder(exprs).aggregate([Agg.count_rows(), Agg.sum("ps"), Agg.sum(col("ps") / col("kn"))], group_by=keys, max_groups=limit)
        assert [k for k, _ in res] == list(groups)
        for (k, got), idx in zip(res, groups.values()):
            ps = [big.rows[i]["ps"] for i in idx if big.rows[i]["ps"] is not None]
            unit = [v for v in (M.agg_row(col("ps") / col("kn"), SCHEMA, big.rows[i]) for i in idx) if v is not None]
            assert got == [len(idx), dec(sum(ps), 2) if ps else None, dec(sum(unit), 6) if unit else None], (keys, limit, k)


def test_top_k_by_a_quotient_then_a_second_key(big):
    e = col("i") // col("kn")
    want, _ = big.model(e)
    for desc, nf in ((False, False), (True, True), (True, False)):
        got = big.builder({"bq": e}).top_k([SortKey("bq", descending=desc, nulls_first=nf), SortKey("id", descending=True)], 40)

        def order(i):
            v = want[i]
            null_rank = (0 if nf else 1) if v is None else (1 if nf else 0)
            return (null_rank, 0 if v is None else (-v if desc else v), -i)
        exp = sorted(range(big.n), key=order)[:40]
        assert got.column("id").to_pylist() == exp and got_values(got, "bq") == [want[i] for i in exp], (desc, nf)


def test_collect_keys_of_a_floor_bucket_used_in_in_set(big):
    e = col("i") // 2 ** 28  # sixteen buckets, some of them negative; NULL where i is
    want, _ = big.model(e)
    small = [i for i in range(1, big.n) if i % 97 == 0][:4]
    ks = big.builder({"bk": e}).with_row_filter(P.in_list("id", [V.Int64(i) for i in small]), prune=False).collect_keys("bk", max_keys=1 << 10)
    try:
        keys = {want[i] for i in small if want[i] is not None}
        assert len(ks) == len(keys) and 1 <= len(keys) <= 4
        t = concat_batches(list(big.builder({"bk": e}).with_row_filter(P.in_set("bk", ks), prune=False).build()))
        assert t.column("id").to_pylist() == [i for i in range(big.n) if want[i] in keys]
    finally:
        ks.close()


def test_c_side_refusals(big):
    def refused(run, code, *fragments):
        with pytest.raises(capi.OrcGpuError) as e:
            run()
        assert e.value.code == code and all(f in str(e.value) for f in fragments), str(e.value)
    refused(lambda: list(big.builder({"r": col("p") // 2}).build()), 6, "//", "column 'p'", "computed column 'r'", "takes integers")
    refused(lambda: list(big.builder({"r": col("i") % col("q")}).build()), 6, "%", "column 'i'")
    refused(lambda: list(big.builder({"r": col("x") % 2.0}).build()), 6, "Float / Double expression", "%")
    refused(lambda: big.builder().aggregate([Agg.sum(col("x") // col("y"))]), 6, "Float / Double expression", "//")
    refused(lambda: list(big.builder({"r": divide("q", "i", scale=1)}).build()), 7, "dividend scale 4", "divisor scale 0", "result scale 1")
    refused(lambda: list(big.builder().with_row_filter((col("p") % 2).eq(1), prune=False).build()), 6, "row filter:", "%", "column 'p'")
    refused(lambda: list(big.builder({"r": year(col("d") / 7)}).build()), 6, "year()", "quotient")
    bad = col("L") / col("M")
    bad.scale = 39  # (what Python's builders never make)
    refused(lambda: list(big.builder({"r": bad}).build()), 101, "names no result scale")
    refused(lambda: list(big.builder().with_row_filter(bad < 1, prune=False).build()), 101, "names no result scale")
    refused(lambda: big.builder().aggregate([Agg.sum(bad)]), 101, "names no result scale")
