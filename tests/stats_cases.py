"""Columns whose statistics sit on the edges the row index kernel (device/col_stats.hip, ix_stats_kernel) and the host merges
(orcgpu_writer_host.inc: wr_stat_merge) decide, shared by the CPU checks (tests/test_writer_stats_reference.py) and the GPU tests
(tests/test_gpu_writer_stats.py).

The kernel gives valid value i of a (column, group) job to thread i mod 256 and then merges threads t and t + d for d = 128, 64,
.., 1; the host merges groups in row order, then stripes.  A case is a list of values in its canonical order; `positions` places
its first half on one side and its second half on the other, in one of PLACEMENTS:

    thread    every value in thread 0 (valid indices 0, 256, 512, ..)
    t0_t1     the halves in threads 0 and 1 (merged at d = 1)
    t3_t131   the halves in threads 3 and 131 (merged at d = 128)
    t5_t0     the halves in threads 5 and 0, the first half at lower valid indices (only there an index tie-break decides)
    groups    the halves in groups 0 and 1 of stripe 0
    stripes   the halves in group 0 of stripes 0 and 1

Every layout is two stripes of two groups of `nv` valid values; with nulls, a null follows every valid value, so a value's row is
twice its valid index.  Positions not taken by a case hold its filler."""
import numpy as np
import pyarrow as pa

PLACEMENTS = ("thread", "t0_t1", "t3_t131", "t5_t0", "groups", "stripes")
_BASES = {"t0_t1": (0, 1), "t3_t131": (3, 131), "t5_t0": (5, 256)}

DBL_MAX = float(np.finfo(np.float64).max)
FLT_MAX = float(np.finfo(np.float32).max)
DBL_TINY = 5e-324  # 2^-1074
FLT_TINY = float(np.float32(2.0 ** -149))
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)


def positions(k, placement):
    """(stripe, group, valid index) of each of k values"""
    h = (k + 1) // 2
    out = []
    for i in range(k):
        s, j = (0, i) if i < h else (1, i - h)
        if placement == "thread":
            out.append((0, 0, 256 * i))
        elif placement in _BASES:
            out.append((0, 0, _BASES[placement][s] + 256 * j))
        elif placement == "groups":
            out.append((0, s, 7 + 256 * j))
        else:
            out.append((s, 0, 7 + 256 * j))
    return out


def nv_for(cases, placement, least=512):
    """valid values per group that hold every case"""
    top = max((max(p[2] for p in positions(len(c["values"]), placement)) for c in cases if c["values"]), default=0)
    return max(least, (top // 256 + 2) * 256)


def column_values(case, placement, nv):
    """the case's valid values in row order: 2 stripes x 2 groups x nv"""
    f = case["filler"]
    v = list(f(nv)) if callable(f) else [f] * (4 * nv)
    for x, (s, g, i) in zip(case["values"], positions(len(case["values"]), placement)):
        v[(2 * s + g) * nv + i] = x
    return v


def layout(cases, typ, placement, nulls):
    """(batches: one per stripe, stride) of a table with a column per case, all of type typ"""
    nv = nv_for(cases, placement)
    stride = 2 * nv if nulls else nv
    cols = {}
    for c in cases:
        v = column_values(c, placement, nv)
        if nulls:
            v = [x for y in v for x in (y, None)]
        cols[c["name"]] = v
    batches = []
    for s in range(2):
        part = {k: v[s * 2 * stride:(s + 1) * 2 * stride] for k, v in cols.items()}
        batches.append(pa.RecordBatch.from_pydict({k: pa.array(x, type=typ) for k, x in part.items()}))
    return batches, stride


# ---- floats: sums ---------------------------------------------------------------------------------------------------------
def _cond_set(k, c, np_t):
    """[B, a, -B, -a, S]: B = 2^k, a = 3/4 ulp(B) (B + a rounds up), S = 2^(k + 1 - c), so sum |x| / |S| is about 2^c; the
    exact sum is S, left-to-right summation gives S + ulp(B) / 4"""
    B, a, S = 2.0 ** k, 3 * 2.0 ** (k - 54), 2.0 ** (k + 1 - c)
    return [np_t(x).item() for x in (B, a, -B, -a, S)]


def float_sum_cases(np_t):
    """(cases, names of the ill-conditioned ones) of a float type (np.float64 or np.float32)"""
    rng = np.random.default_rng(20 if np_t is np.float64 else 21)
    f32 = np_t is np.float32
    cases = []
    x = [np_t(rng.uniform(1, 2) * 2.0 ** rng.integers(0, 60)).item() for _ in range(8)]
    r = [float(y) for y in rng.integers(1, 5, 8) * rng.choice([-1, 1], 8)]
    cases.append({"name": "cancel_pairs", "values": x + [np_t(-a + b).item() for a, b in zip(x, r)], "filler": 0.0})
    big = np_t(1e16).item()
    cases.append({"name": "ones", "values": [big] + [1.0] * 30 + [-big], "filler": 0.0})
    k = 100 if f32 else 700
    for c, name in ((27, "cond1e8"), (54, "cond1e16"), (80, "cond1e24"), (100, "cond1e30")):
        cases.append({"name": name, "values": _cond_set(k, c, np_t), "filler": 0.0})
    ill = [c["name"] for c in cases]
    if not f32:  # (B in the scaled accumulator, a and S in the other)
        cases.append({"name": "cond1e16_big", "values": _cond_set(1000, 54, np_t), "filler": 0.0})
        cases += [
            {"name": "ovf_pair", "values": [1.5e308, 1.5e308], "filler": 0.0},
            {"name": "ovf_three", "values": [1.79e308] * 3, "filler": 1.0},
            {"name": "ovf_neg", "values": [-1.2e308] * 4, "filler": -1.0},
            {"name": "ovf_mixed", "values": [1.5e308, 1.5e308, -1e308, -1.9e308], "filler": 0.0},
            {"name": "ovf_mixed_small", "values": [1.7e308, 1.6e308, 0.25, -1.6e308, -1.7e308], "filler": 1.0},
            {"name": "ovf_then_ninf", "values": [1.7e308, 1.7e308, -np.inf], "filler": 0.0},
        ]
    else:
        cases.append({"name": "flt_max", "values": [FLT_MAX] * 4, "filler": FLT_MAX})
    cases += [
        {"name": "inf", "values": [np.inf, 1.0], "filler": 2.0},
        {"name": "inf_both", "values": [np.inf, -np.inf], "filler": 0.0},
    ]
    tiny = FLT_TINY if f32 else DBL_TINY
    q = rng.integers(-(1 << 22), 1 << 22, 1 << 14) if f32 else rng.integers(-(1 << 51), 1 << 51, 1 << 14)
    sub = [np_t(float(y) * tiny).item() for y in q]
    cases.append({"name": "subnormal_sum", "values": [], "filler": lambda nv: (sub * (4 * nv // len(sub) + 1))[:4 * nv]})
    return cases, ill


SUBNORMAL_SUMS = ("subnormal_sum",)


# ---- floats: minimum and maximum --------------------------------------------------------------------------------------------
def _starts_with(z):
    def f(nv):
        v = [-z] * (4 * nv)
        v[::nv] = [z] * 4
        return v
    return f


def float_minmax_cases(np_t):
    f32 = np_t is np.float32
    tiny = FLT_TINY if f32 else DBL_TINY
    top = FLT_MAX if f32 else DBL_MAX
    return [
        {"name": "zeros_pos_first", "values": [], "filler": _starts_with(0.0)},
        {"name": "zeros_neg_first", "values": [], "filler": _starts_with(-0.0)},
        {"name": "min_neg_zero_first", "values": [-0.0, 0.0], "filler": 1.5},
        {"name": "min_pos_zero_first", "values": [0.0, -0.0], "filler": 1.5},
        {"name": "max_neg_zero_first", "values": [-0.0, 0.0], "filler": -1.5},
        {"name": "max_pos_zero_first", "values": [0.0, -0.0], "filler": -1.5},
        {"name": "tiny_both", "values": [-tiny, tiny], "filler": 0.0},
        {"name": "tiny_min", "values": [2 * tiny, tiny], "filler": 1.0},
        {"name": "tiny_max", "values": [-2 * tiny, -tiny], "filler": -1.0},
        {"name": "extremes", "values": [top, -top], "filler": 0.5},
    ]


# ---- integers -----------------------------------------------------------------------------------------------------------------
def int64_cases():
    return [
        {"name": "wrap_3", "values": [I64_MAX, I64_MAX, I64_MIN, I64_MIN, 5], "filler": 0},
        {"name": "halves_absent", "values": [I64_MAX, I64_MAX, I64_MIN, I64_MIN], "filler": 0},
        {"name": "sum_max", "values": [I64_MAX - 1000, 1000], "filler": 0},
        {"name": "sum_max_plus1", "values": [I64_MAX - 1000, 1001], "filler": 0},
        {"name": "sum_min", "values": [I64_MIN + 1000, -1000], "filler": 0},
        {"name": "sum_min_minus1", "values": [I64_MIN + 1000, -1001], "filler": 0},
        {"name": "extremes", "values": [I64_MIN, I64_MAX], "filler": 3},
    ]


# compared with Apache ORC C++: whole statistics where its running sums stay inside i64 (it drops a sum at its first overflow,
# merges included), the minimum and maximum alone for "extremes"
CPP_SAFE_INT64 = ("sum_max", "sum_min")
CPP_BOUNDS_INT64 = ("extremes",)


def small_int_table(nv, rng):
    """Int8 / Int16 / Int32 extremes over 4 nv values (groups of nv: the per-thread loop runs nv / 256 times).  Int16 and Int32
    mix both ends: the writer's Integer RLE v2 encoder (as the reference's) writes some runs of values near their type's limits
    wrongly (constant runs of more than 10 values, for one), which is not a statistics matter"""
    cols = {}
    n = 4 * nv
    for t in (np.int8, np.int16, np.int32):
        lo, hi = int(np.iinfo(t).min), int(np.iinfo(t).max)
        if t is np.int8:
            cols["int8_max"] = pa.array(np.full(n, hi, dtype=t))
            cols["int8_min"] = pa.array(np.full(n, lo, dtype=t))
        cols["%s_mix" % t.__name__] = pa.array(rng.choice(np.array([lo, hi, lo + 1, hi - 1], dtype=t), n), mask=rng.random(n) < 0.2)
    return cols


# ---- strings --------------------------------------------------------------------------------------------------------------
def _prefix(n, seed):
    r = np.random.default_rng(seed)
    return "".join(chr(c) for c in r.integers(ord("a"), ord("z") + 1, n))


def string_cases(long=True):
    cases = []
    for L in (8, 9, 16, 1023):
        p = _prefix(L, L)
        cases.append({"name": "prefix%d" % L, "values": [p + "c", p + "a"], "filler": p + "b"})
    cases += [
        {"name": "nul_tail", "values": ["ab\x00\x00", "ab", "", "ab\x00"], "filler": "ab\x00"},
        {"name": "nul_min_ab", "values": ["ab\x00\x00", "ab"], "filler": "ab\x00"},
        {"name": "empty_min", "values": ["ab", ""], "filler": "ab"},
        {"name": "high_byte", "values": ["\x7fz", "éa"], "filler": "\x7f{"},
        {"name": "high_byte_rev", "values": ["éa", "\x7fz"], "filler": "\x7f{"},
    ]
    if long:
        P = _prefix(2000, 2000)
        cases += [
            {"name": "long_a", "values": [P, P[:1024], P[:1026], P[:1023], P[:1025]], "filler": P[:1023]},
            {"name": "long_b", "values": [P[:1024], P[:1023], P[:1025], P, P[:1026]], "filler": P[:1023]},
            {"name": "long_c", "values": [P[:1025], P[:1026], P[:1024], P[:1023]], "filler": P[:1023]},
        ]
    return cases
