"""The statistics reference (tests/index_model.py) checks itself, no GPU:

- FloatSum's R is the exact sum rounded to nearest: math.fsum wherever fsum does not raise, +-inf where the exact sum is beyond f64;
- on every float input of tests/test_gpu_writer_stats.py, a plain double-double reduction meets FloatSum.tol -- the reduction in
  the device's order (256 threads, tree, host merges) at every range too -- and left-to-right summation misses it by at least
  100 times on every ill-conditioned case (else the case would prove nothing);
- the model's minima, maxima and integer statistics are what Apache ORC C++ (pyarrow's writer) records for the same columns."""
import io
import math

import numpy as np
import pyarrow as pa
import pyarrow.orc as po
import pytest

import index_model as IM
import stats_cases as SC
from orcfile import OrcFile

F_TYPES = {"f64": (np.float64, pa.float64()), "f32": (np.float32, pa.float32())}


def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def dd_add(h, l, x):
    s, e = two_sum(h, x)
    return s, l + e


def dd_merge(h, l, h2, l2):
    if not (math.isfinite(h) and math.isfinite(h2)):
        return h + h2, 0.0
    s, e = two_sum(h, h2)
    e += l + l2
    hi = s + e
    return hi, e - (hi - s)


class Acc:
    """the writer's float sum: two double-doubles, values below 2^960 in magnitude and the others scaled by 2^-64"""

    def __init__(self):
        self.s = (0.0, 0.0)
        self.b = (0.0, 0.0)

    def add(self, x):
        if abs(x) < 2.0 ** 960:
            self.s = dd_add(*self.s, x)
        elif math.isfinite(self.b[0]):
            self.b = dd_add(*self.b, x * 2.0 ** -64)
        else:
            self.b = (self.b[0] + x, self.b[1])

    def merge(self, o):
        self.s = dd_merge(*self.s, *o.s)
        self.b = dd_merge(*self.b, *o.b)

    def value(self):
        bh, bl = self.b
        if not math.isfinite(bh):
            return bh
        if bh == 0 and bl == 0:
            return self.s[0] + self.s[1]
        h, l = dd_merge(bh, bl, math.ldexp(self.s[0], -64), math.ldexp(self.s[1], -64))
        try:
            return math.ldexp(h + l, 64)
        except OverflowError:
            return math.copysign(math.inf, h)


def seq_sum(vals):
    a = Acc()
    for x in vals:
        a.add(x)
    return a.value()


def naive(vals):
    s = 0.0
    for x in vals:
        s += x
    return s


def device_group(vals):
    """one group as ix_stats_kernel reduces it: valid value i in thread i mod 256, then the tree"""
    th = [Acc() for _ in range(256)]
    for i, x in enumerate(vals):
        th[i % 256].add(x)
    d = 128
    while d:
        for t in range(d):
            th[t].merge(th[t + d])
        d //= 2
    return th[0]


def _sum_inputs():
    """(name, values) of every float range the GPU tests reduce: each case's canonical order, and per placement each group, stripe
    and the file"""
    for tname, (np_t, _) in F_TYPES.items():
        for cases in (SC.float_sum_cases(np_t)[0], SC.float_minmax_cases(np_t)):
            for c in cases:
                if c["values"]:
                    yield "%s/%s" % (tname, c["name"]), c["values"], None
                for pl in SC.PLACEMENTS:
                    nv = SC.nv_for(cases, pl)
                    v = SC.column_values(c, pl, nv)
                    yield "%s/%s/%s" % (tname, c["name"], pl), v, [v[k * nv:(k + 1) * nv] for k in range(4)]


def test_float_sum_is_rounded_exact_sum():
    """R == fsum wherever fsum does not raise; +-inf where the exact sum overflows; the infinity rules"""
    n_ovf = 0
    for name, v, _ in _sum_inputs():
        if any(math.isinf(x) for x in v):
            continue
        R = IM.FloatSum(v)
        try:
            f = math.fsum(v)
        except OverflowError:  # (fsum raises on an intermediate overflow too: then the exact sum may be finite)
            n_ovf += 1
            if "ovf_mixed" in name:
                assert abs(R.exact) <= IM.fixed(SC.DBL_MAX) // 2 and R == IM.Fraction(R.exact, IM.ULP0), name
            else:
                assert math.isinf(R) and (R > 0) == (R.exact > 0), name
                assert abs(R.exact) >= 2 * IM.fixed(SC.DBL_MAX) or "ovf_pair" in name, name
            continue
        assert R == f and math.copysign(1, R) == math.copysign(1, f) or R == f == 0, (name, R, f)
    assert n_ovf >= 6
    assert IM.FloatSum([1.5e308, 1.5e308]) == math.inf and IM.FloatSum([-1.5e308, -1.5e308]) == -math.inf
    assert IM.FloatSum([SC.DBL_MAX, SC.DBL_MAX, -SC.DBL_MAX]) == SC.DBL_MAX
    assert IM.FloatSum([1.7e308, 1.7e308, -math.inf]) == -math.inf
    assert math.isnan(IM.FloatSum([math.inf, 1.0, -math.inf]))
    assert IM.FloatSum([math.inf, 1e308, 1e308]) == math.inf
    # the bound: exact where nothing rounds, in Fractions for subnormal and overflowing ranges
    assert IM.FloatSum([1.0, 2.0]).tol() > 0 and IM.FloatSum([0.0, -0.0]).tol() == 0
    assert IM.FloatSum([5e-324, 5e-324]).tol() > 0 and IM.FloatSum([1.7e308] * 3).tol() > 0
    # same_stats holds sums to R's contract
    st = {"n": 2, "has_null": False, "double": (1.5e308, 1.5e308, IM.FloatSum([1.5e308, 1.5e308]))}
    assert IM.same_stats({"n": 2, "has_null": False, "double": (1.5e308, 1.5e308, math.inf)}, st)
    assert not IM.same_stats({"n": 2, "has_null": False, "double": (1.5e308, 1.5e308, math.nan)}, st)
    st = {"n": 3, "has_null": False, "double": (-1e16, 1e16, IM.FloatSum([1e16, 1.0, -1e16]))}
    assert IM.same_stats({"n": 3, "has_null": False, "double": (-1e16, 1e16, 1.0)}, st)
    assert not IM.same_stats({"n": 3, "has_null": False, "double": (-1e16, 1e16, 0.0)}, st)
    assert not IM.same_stats({"n": 3, "has_null": False, "double": (-1e16, 1e16, math.nan)}, st)


def test_double_double_meets_tol():
    """a plain double-double (Acc) meets tol on every input, sequentially and in the device's order at every range"""
    checked = 0
    for name, v, groups in _sum_inputs():
        R = IM.FloatSum(v)
        assert R.admits(seq_sum(v)), (name, seq_sum(v), R)
        if groups is None:
            continue
        accs = [device_group(g) for g in groups]
        for k, a in enumerate(accs):
            assert IM.FloatSum(groups[k]).admits(a.value()), (name, k, a.value())
        stripes = []
        for s in range(2):
            a = Acc()
            a.merge(accs[2 * s])
            a.merge(accs[2 * s + 1])
            assert IM.FloatSum(groups[2 * s] + groups[2 * s + 1]).admits(a.value()), (name, s, a.value())
            stripes.append(a)
        f = Acc()
        f.merge(stripes[0])
        f.merge(stripes[1])
        assert R.admits(f.value()), (name, f.value(), R)
        checked += 1
    assert checked > 100


@pytest.mark.parametrize("tname", list(F_TYPES))
def test_naive_sum_misses_ill_conditioned(tname):
    """left-to-right summation misses tol by at least 100x on every ill-conditioned case, and the condition numbers are what the
    cases are named for (within a factor of 2)"""
    cases, ill = SC.float_sum_cases(F_TYPES[tname][0])
    for c in cases:
        if c["name"] not in ill:
            continue
        v = c["values"]
        R = IM.FloatSum(v)
        err = abs(IM.Fraction(naive(v)) - R.S())
        assert err >= 100 * R.tol(), (c["name"], float(err), float(R.tol()))
        if c["name"].startswith("cond"):
            cond = float(R.abs_sum / R.exact)
            target = float(c["name"][4:])
            assert target / 2 <= cond <= target * 2, (c["name"], cond)


def _cpp_stats(table, stride):
    buf = io.BytesIO()
    po.write_table(table, buf, row_index_stride=stride, compression="uncompressed", stripe_size=1 << 30)
    of = OrcFile(buf.getvalue())
    rows = [s.number_of_rows for s in of.stripes]
    groups, stripes, whole = IM.model_groups(table, rows, stride)
    got = []
    for si, s in enumerate(of.stripes):
        for col in range(1, table.num_columns + 1):
            entries = IM.row_index_entries(of, s, col)
            assert len(entries) == len(groups[si])
            got += [((si, g, col), st, groups[si][g][col]) for g, (_, st) in enumerate(entries)]
    fstats, sstats = IM.file_statistics(of)
    for si, ss in enumerate(sstats):
        got += [((si, "stripe", col), ss[col], stripes[si][col]) for col in range(1, table.num_columns + 1)]
    got += [(("file", col), fstats[col], whole[col]) for col in range(1, table.num_columns + 1)]
    return got


def _same_bounds(got, want, key):
    if key == "double":
        (a0, a1, _), (b0, b1, _) = got, want  # (C++ sums naively: sums are not compared)
        return a0 == b0 and a1 == b1 and math.copysign(1, a0) == math.copysign(1, b0) and math.copysign(1, a1) == math.copysign(1, b1)
    if key == "string":
        return (got[0], got[1], got[4]) == (want[0], want[1], want[4])
    return got == want


def _table(batches):
    return pa.Table.from_batches(batches)


@pytest.mark.parametrize("placement", SC.PLACEMENTS)
def test_model_against_cpp(placement):
    """floats (signed zeros, subnormals, extremes), strings of at most 1024 bytes and integers: pyarrow's writer (Apache ORC C++)
    records the model's minimum and maximum (and the integers' sums) in every group, stripe and the file"""
    import oracle_lib as O
    O.lib()
    tables = []
    for tname, (np_t, typ) in F_TYPES.items():
        cases = SC.float_minmax_cases(np_t) + [c for c in SC.float_sum_cases(np_t)[0] if not c["name"].startswith("ovf")]
        for nulls in (False, True):
            b, stride = SC.layout(cases, typ, placement, nulls)
            tables.append((_table(b), stride, "double"))
    for typ in (pa.string(), pa.large_string()):
        b, stride = SC.layout(SC.string_cases(long=False), typ, placement, True)
        tables.append((_table(b), stride, "string"))
    ints = [c for c in SC.int64_cases() if c["name"] in SC.CPP_SAFE_INT64 + SC.CPP_BOUNDS_INT64]
    b, stride = SC.layout(ints, pa.int64(), placement, True)
    tables.append((_table(b), stride, "int"))
    checked = 0
    for t, stride, key in tables:
        for where, st, want in _cpp_stats(t, stride):
            assert st["n"] == want["n"] and st["has_null"] == want["has_null"], (key, where)
            if key in want:
                name = t.column_names[where[-1] - 1]
                g, w = st.get(key), want[key]
                if key == "int" and name in SC.CPP_BOUNDS_INT64:
                    g, w = g[:2], w[:2]
                assert g is not None and _same_bounds(g, w, key), (key, where, name, g, w)
                checked += 1
    assert checked > 100


def test_model_against_cpp_small_ints():
    import oracle_lib as O
    O.lib()
    rng = np.random.default_rng(22)
    t = pa.table(SC.small_int_table(4096, rng))
    checked = 0
    for where, st, want in _cpp_stats(t, 4096):
        assert st["n"] == want["n"] and st["int"] == want["int"], (where, st, want)
        checked += 1
    assert checked > 20
