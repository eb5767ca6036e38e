"""Row index statistics at the edges the GPU decides (device/col_stats.hip: ix_stats_kernel; orcgpu_writer_host.inc: wr_stat_merge,
wr_float_sum): every group's, stripe's and the file's statistics against tests/index_model.py, whose float sums are the exact sum
rounded to nearest, held to FloatSum.tol.  The columns are tests/stats_cases.py's, each placed in one thread, in threads merged
last and first in the tree, in threads whose first value sits in the higher thread, in two groups and in two stripes, with and
without nulls between the values."""
import numpy as np
import pyarrow as pa
import pytest

import index_model as IM
import stats_cases as SC
from orcfile import OrcFile
from test_gpu_writer_index import check_index, write

pytestmark = pytest.mark.gpu

F_TYPES = {"f64": (np.float64, pa.float64()), "f32": (np.float32, pa.float32())}


def _write_check(batches, stride, comp=None):
    data, rows, _ = write(batches, stride, comp, flush_after=(0,))
    assert len(rows) == 2
    check_index(data, pa.Table.from_batches(batches), rows, stride)
    return data, rows


def _double_sums(data, table, rows, stride, col):
    """(got, want) double sums of one column (1-based) at every group, stripe and the file"""
    of = OrcFile(data)
    groups, stripes, whole = IM.model_groups(table, rows, stride)
    out = []
    for si, s in enumerate(of.stripes):
        for g, (_, st) in enumerate(IM.row_index_entries(of, s, col)):
            out.append((st["double"][2], groups[si][g][col]["double"][2]))
    fstats, sstats = IM.file_statistics(of)
    out += [(ss[col]["double"][2], stripes[si][col]["double"][2]) for si, ss in enumerate(sstats)]
    out.append((fstats[col]["double"][2], whole[col]["double"][2]))
    return out


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("placement", SC.PLACEMENTS)
@pytest.mark.parametrize("tname", list(F_TYPES))
def test_float_sums(tname, placement, nulls):
    """ill-conditioned sets, overflowing sums (one sign: that infinity, never NaN; mixed signs: finite within tol), infinite inputs;
    subnormal-only sums equal R exactly"""
    np_t, typ = F_TYPES[tname]
    cases, _ = SC.float_sum_cases(np_t)
    batches, stride = SC.layout(cases, typ, placement, nulls)
    data, rows = _write_check(batches, stride)
    table = pa.Table.from_batches(batches)
    for name in SC.SUBNORMAL_SUMS:
        col = table.column_names.index(name) + 1
        for got, want in _double_sums(data, table, rows, stride, col):
            assert got == want, (name, got, want)


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("placement", SC.PLACEMENTS)
@pytest.mark.parametrize("tname", list(F_TYPES))
def test_float_minmax(tname, placement, nulls):
    """signed zeros (the first of equal values), subnormal and largest finite bounds"""
    np_t, typ = F_TYPES[tname]
    batches, stride = SC.layout(SC.float_minmax_cases(np_t), typ, placement, nulls)
    _write_check(batches, stride)


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("placement", SC.PLACEMENTS)
def test_int64_sums(placement, nulls):
    """exact sums whose partial sums leave i64; sums of exactly INT64_MAX / INT64_MIN and one past each"""
    batches, stride = SC.layout(SC.int64_cases(), pa.int64(), placement, nulls)
    _write_check(batches, stride)


def test_small_int_extremes():
    """Int8 / Int16 / Int32 extremes over groups of 4096 values (16 values a thread)"""
    rng = np.random.default_rng(30)
    cols = SC.small_int_table(4096, rng)
    t = pa.table(cols)
    batches = [t.slice(0, 8192).to_batches()[0], t.slice(8192).to_batches()[0]]
    _write_check(batches, 4096)


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("placement", SC.PLACEMENTS)
@pytest.mark.parametrize("typ", [pa.string(), pa.large_string()], ids=["utf8", "large_utf8"])
def test_strings(typ, placement, nulls):
    """ties on the 8-byte key: shared prefixes of 8, 9, 16 and 1023 bytes, NUL tails, first bytes on both sides of 0x80, and
    lengths 1023 to 2000 sharing 1025 bytes whose bound the host settles"""
    batches, stride = SC.layout(SC.string_cases(), typ, placement, nulls)
    _write_check(batches, stride)


def _stride_table(S, rng):
    """about 3.5 groups of S rows: group 1 without valid values, group 2 with exactly one, random nulls elsewhere"""
    n = 3 * S + max(1, S // 2)
    mask = rng.random(n) < 0.3
    mask[S:2 * S] = True
    mask[2 * S:3 * S] = True
    mask[2 * S + (S - 1) // 2] = False
    f = rng.standard_normal(n) * 10.0 ** rng.integers(-20, 20, n)
    f[rng.integers(0, n, 4)] = [0.0, -0.0, SC.DBL_TINY, -SC.DBL_MAX]
    i = rng.integers(-(1 << 62), 1 << 62, n)
    i[rng.integers(0, n, 3)] = [SC.I64_MAX, SC.I64_MIN, SC.I64_MAX]
    s = ["%x" % x for x in rng.integers(0, 1 << 40, n)]
    for k in rng.integers(0, n, 3):
        s[k] = "pfx_common_" + "\xe9" * int(rng.integers(0, 600))
    return pa.table({
        "i64": pa.array(i, mask=mask),
        "i32": pa.array(rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32), mask=mask),
        "f64": pa.array(f, mask=mask),
        "f32": pa.array(np.clip(f, -SC.FLT_MAX, SC.FLT_MAX).astype(np.float32), mask=mask),
        "s": pa.array(s, mask=mask),
        "ls": pa.array(s, type=pa.large_string(), mask=mask),
    })


@pytest.mark.parametrize("stride", [1, 255, 256, 257, 1000, 4096, 65537])
def test_strides(stride):
    """group shapes around the block size: a group without valid values, one with exactly one, nulls between the values"""
    rng = np.random.default_rng(stride)
    S = stride if stride > 1 else 300
    t = _stride_table(S, rng)
    cut = 2 * S  # (stripe 0: a random group and the empty one; stripe 1 starts with the group of one valid value)
    batches = [t.slice(0, cut).to_batches()[0], t.slice(cut).to_batches()[0]]
    _write_check(batches, stride)


def _family(fam):
    if fam == "float_sums":
        return SC.float_sum_cases(np.float64)[0], pa.float64()
    if fam == "float_minmax":
        return SC.float_minmax_cases(np.float32), pa.float32()
    if fam == "int64":
        return SC.int64_cases(), pa.int64()
    return SC.string_cases(), pa.string()


@pytest.mark.parametrize("comp", ["snappy", "lz4"])
@pytest.mark.parametrize("fam", ["float_sums", "float_minmax", "int64", "strings"])
def test_compressed_same_statistics(fam, comp):
    """compression does not change the statistics"""
    cases, typ = _family(fam)
    batches, stride = SC.layout(cases, typ, "t5_t0", True)
    plain, _ = _write_check(batches, stride)
    data, _ = _write_check(batches, stride, comp)
    p, d = OrcFile(plain), OrcFile(data)
    assert repr(IM.file_statistics(p)) == repr(IM.file_statistics(d))
    for s0, s1 in zip(p.stripes, d.stripes):
        for col in range(len(cases) + 1):
            e0, e1 = IM.row_index_entries(p, s0, col), IM.row_index_entries(d, s1, col)
            assert repr([st for _, st in e0]) == repr([st for _, st in e1])
