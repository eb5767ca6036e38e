"""Key maps and lookup columns on the GPU (ArrowReaderBuilder.collect_map / with_lookup_columns; key_map_insert_kernel and
lookup_columns_kernel in device/key_map_kernels.hip) against the dict of tests/key_map_model.py, row for row and exactly: integers
and Decimals as Python ints, doubles by their bits.  Files are written in the test with pyarrow, a few thousand rows at most; a
side of more than 1024 rows under a tiny stripe_size is cut into stripes of 1024 rows.  Every test here needs collect_map: none
passes without the feature."""
import decimal
import os
import re

import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

import agg_expr_model as AEM
import key_map_model as M
import test_gpu_aggregate as TA
import top_k_model as TK
from orc_rust_amd import KeyMap, capi
from orc_rust_amd.aggregate import Agg, col
from orc_rust_amd.arrow_reader import ArrowReaderBuilder, concat_batches
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
from orc_rust_amd.top_k import SortKey

pytestmark = pytest.mark.gpu

D = decimal.Decimal
EXACT = decimal.Context(prec=80)
BATCH = 1024
UNSUPPORTED, MISMATCHED, INVALID = 7, 6, 101
# the build side's value columns: name -> (arrow type, what the map hands it out as)
VALUES = {"v8": (pa.int8(), pa.int64()), "v32": (pa.int32(), pa.int64()), "v64": (pa.int64(), pa.int64()), "vd": (pa.date32(), pa.int64()),
          "vp": (pa.decimal128(12, 2), pa.decimal128(12, 2)), "vw": (pa.decimal128(38, 0), pa.decimal128(38, 0)), "vf32": (pa.float32(), pa.float64()),
          "vf64": (pa.float64(), pa.float64())}
ALL = list(VALUES)  # eight values at once
_CTX = None


def ctx():
    global _CTX
    if _CTX is None:
        _CTX = capi.Context()
    return _CTX


def dec(unscaled, scale):
    return D(unscaled).scaleb(-scale, EXACT)


def write(tmpdir, name, table, stripes=1):
    """`table` as an ORC file: one stripe, or -- under a tiny stripe_size -- stripes of 1024 rows each but the last"""
    path = str(tmpdir / (name + ".orc"))
    orc.write_table(table, path, compression="uncompressed", row_index_stride=1000, stripe_size=(64 << 20) if stripes == 1 else 1024)
    assert stripes == 1 or orc.ORCFile(path).nstripes == (table.num_rows + 1023) // 1024 == stripes, (name, orc.ORCFile(path).nstripes)
    return path


def arrow_column(values, typ):
    if pa.types.is_decimal(typ):
        return pa.array([None if v is None else dec(v, typ.scale) for v in values], typ)
    if pa.types.is_date(typ):
        return pa.array(values, pa.int32()).cast(typ)
    return pa.array(values, typ)


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


def spell(name, values):
    return [None if v is None else M.bits(v) for v in values] if name.startswith("vf") else values


class Build:
    """A build side: rows of (k, f, the eight value columns); the keys distinct unless the caller says otherwise"""

    def __init__(self, tmpdir, name, keys, stripes=1, key_type=pa.int64(), null_keys=(), seed=3):
        n = len(keys)
        rng = np.random.default_rng(seed + n)
        self.n = n
        self.keys = [None if i in null_keys else int(k) for i, k in enumerate(keys)]
        self.f = [i % 10 for i in range(n)]

        def nulls(values):
            return [None if (m or i == 0) and n > 2 else v for i, (v, m) in enumerate(zip(values, rng.random(n) < 0.2))]

        c = {"v8": nulls([int(v) for v in rng.integers(-128, 128, n)]), "v32": nulls([int(v) for v in rng.integers(-2 ** 31, 2 ** 31, n)]),
             "v64": [int(v) for v in rng.integers(-2 ** 62, 2 ** 62, n)],  # (no NULL: no PRESENT stream)
             "vd": nulls([int(v) for v in rng.integers(-1000, 20000, n)]), "vp": nulls([int(v) for v in rng.integers(-10 ** 11, 10 ** 11, n)]),
             "vw": nulls([[10 ** 38 - 1, 1 - 10 ** 38, 0, 2 ** 64, -7][int(v)] for v in rng.integers(0, 5, n)]),
             "vf32": nulls([float(v) / 4 for v in rng.integers(-4000, 4000, n)]),
             "vf64": nulls([[0.1, -0.0, float("inf"), 1e-320, 1.5, 0.30000000000000004][int(v)] for v in rng.integers(0, 6, n)])}
        self.c = c
        cols = {"k": pa.array(self.keys, key_type), "f": pa.array(self.f, pa.int64())}
        for v, (typ, _) in VALUES.items():
            cols[v] = arrow_column(c[v], typ)
        self.path = write(tmpdir, name, pa.table(cols), stripes)

    def builder(self, f_below=None, prefetch=0):
        b = ArrowReaderBuilder.try_new(self.path, ctx()).with_batch_size(BATCH).with_prefetch(prefetch)
        if f_below is not None:
            b = b.with_row_filter(P.lt("f", V.Int64(f_below)), prune=False)
        return b

    def model(self, values=ALL, f_below=None):
        kept = None if f_below is None else [f < f_below for f in self.f]
        return M.build(self.keys, [tuple(self.c[v][i] for v in values) for i in range(self.n)], kept)

    def collect(self, values=ALL, max_keys=1 << 13, f_below=None, into=None, prefetch=0):
        return self.builder(f_below, prefetch).collect_map("k", list(values), max_keys=max_keys, into=into)


class Probe:
    """A probe side: id, fk (Long, NULLs at word edges), fk32 (Int, no NULL: no PRESENT stream), c"""

    def __init__(self, tmpdir, name, fk, stripes=1, seed=11):
        n = len(fk)
        rng = np.random.default_rng(seed + n)
        self.n = n
        self.fk = [None if (i in (0, 63, 64, 127, 128, n - 1) and i % 2 == 0 and n > 1) else int(k) for i, k in enumerate(fk)]
        self.fk32 = [int(k) if -2 ** 31 <= int(k) < 2 ** 31 else 0 for k in fk]
        self.c = [int(v) for v in rng.integers(0, 10, n)]
        table = pa.table({"id": pa.array(range(n), pa.int64()), "fk": pa.array(self.fk, pa.int64()), "fk32": pa.array(self.fk32, pa.int32()), "c": pa.array(self.c, pa.int64())})
        self.path = write(tmpdir, name, table, stripes)

    def builder(self, prefetch=0):
        return ArrowReaderBuilder.try_new(self.path, ctx()).with_batch_size(BATCH).with_prefetch(prefetch)


def lookups(values=ALL, prefix="o_"):
    return {prefix + v: v for v in values}


def check_probe(table, m, probe_keys, values=ALL, prefix="o_", keep=None):
    """every lookup column of `table` against the model, row for row"""
    for i, v in enumerate(values):
        want = spell(v, M.probe(m, probe_keys, i))
        if keep is not None:
            want = [w for w, ok in zip(want, keep) if ok]
        assert got_values(table, prefix + v) == want, v


@pytest.fixture(scope="module")
def tmpdir(tmp_path_factory):
    capi.load()
    return tmp_path_factory.mktemp("key_map")


def spread(n, seed=1):
    """n distinct keys: small ones and ones spread over int64"""
    rng = np.random.default_rng(seed)
    keys = list(range(-(n // 2), n - n // 2))
    for i in range(0, n, 3):
        keys[i] = int(rng.integers(-2 ** 62, 2 ** 62)) * 2 + 1 + 2 ** 40
    assert len(set(keys)) == n
    return keys


@pytest.fixture(scope="module")
def side(tmpdir):
    """a build side of 65 keys with its sealed map (all eight values), and a probe side of three stripes, the last of one row"""
    b = Build(tmpdir, "side_build", spread(65))
    rng = np.random.default_rng(5)
    fk = [b.keys[int(i)] if h else int(i) + 1000 for i, h in zip(rng.integers(0, 65, 2049), rng.random(2049) < 0.6)]
    p = Probe(tmpdir, "side_probe", fk, stripes=3)
    km = b.collect()
    yield b, p, km
    km.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 4097])
def test_build_side_sizes(tmpdir, side, n):
    b = Build(tmpdir, "b%d" % n, spread(n, seed=n), stripes=(n + 1023) // 1024, null_keys=(n // 2,) if n > 2 else ())
    m, has_null = b.model()
    _, p, _ = side
    fk = [b.keys[i % n] if i % 3 and b.keys[i % n] is not None else i + 10 ** 6 for i in range(p.n)]
    pr = Probe(tmpdir, "pb%d" % n, fk, stripes=3)
    with b.collect() as km:
        assert (len(km), km.has_null, km.rows_seen) == (len(m), has_null, n)
        assert km.value_names == ALL and km.value_types == ["int64"] * 4 + [("decimal128", 12, 2), ("decimal128", 38, 0), "float64", "float64"]
        reader = pr.builder().with_lookup_columns(km, "fk", lookups()).build()
        batches = list(reader)
        for bt in batches:
            bt.validate(full=True)
            assert bt.schema.names == ["id", "fk", "fk32", "c"] + ["o_" + v for v in ALL]
            for v in ALL:
                fld = bt.schema.field("o_" + v)
                assert fld.nullable and fld.type == VALUES[v][1], fld
        assert reader.column_names() == ["id", "fk", "fk32", "c"] + ["o_" + v for v in ALL]
        table = concat_batches(batches)
        assert table.num_rows == pr.n
        check_probe(table, m, pr.fk)


@pytest.mark.parametrize("n, stripes", [(1, 1), (64, 1), (65, 1), (1023, 1), (1024, 1), (1025, 1), (1025, 2), (2049, 1), (2049, 3)])
def test_probe_side_sizes(tmpdir, side, n, stripes):
    b, _, km = side
    m, _ = b.model()
    fk = [b.keys[(i * 7) % 65] if i % 4 else i + 5000 for i in range(n)]
    pr = Probe(tmpdir, "pp%d_%d" % (n, stripes), fk, stripes=stripes)
    table = concat_batches(list(pr.builder().with_lookup_columns(km, "fk", lookups()).build()))
    assert table.num_rows == n
    check_probe(table, m, pr.fk)
    # a probe key column without a PRESENT stream
    t32 = concat_batches(list(pr.builder().with_lookup_columns(km, "fk32", {"x": "v64", "y": "vf64"}).build()))
    assert got_values(t32, "x") == M.probe(m, pr.fk32, ALL.index("v64")) and got_values(t32, "y") == spell("vf64", M.probe(m, pr.fk32, ALL.index("vf64")))


def test_the_three_ways_to_null_are_all_there(side):
    b, p, _ = side
    m, _ = b.model()
    ways = {M.why_null(m, k, ALL.index("v32")) for k in p.fk}
    assert ways == {None, "key", "absent", "value"}


def test_probe_outcomes(tmpdir, side):
    b, p, km = side
    m, _ = b.model()
    none = Probe(tmpdir, "p_none", [10 ** 9 + i for i in range(130)])
    t = concat_batches(list(none.builder().with_lookup_columns(km, "fk", lookups(["v64", "vp"])).build()))
    assert got_values(t, "o_v64") == [None] * 130 and got_values(t, "o_vp") == [None] * 130
    one = Probe(tmpdir, "p_one", [b.keys[7]] * 130)
    t = concat_batches(list(one.builder().with_lookup_columns(km, "fk", lookups()).build()))
    check_probe(t, m, one.fk)
    assert got_values(t, "o_v64").count(m[b.keys[7]][2]) == sum(k is not None for k in one.fk)


@pytest.mark.parametrize("keys", [[M.SENTINEL], [5, M.SENTINEL, -9, M.SENTINEL + 1, M.INT64_MIN, M.INT64_MAX], [5, -9, M.SENTINEL + 1]], ids=["alone", "among", "absent"])
def test_the_sentinels_value_as_a_key(tmpdir, keys):
    b = Build(tmpdir, "bs%d" % len(keys), keys)
    m, _ = b.model()
    pr = Probe(tmpdir, "ps%d" % len(keys), [M.SENTINEL, 5, M.SENTINEL + 1, M.SENTINEL - 1, M.INT64_MIN, 0] * 11 + [M.SENTINEL] * 3)
    with b.collect(max_keys=8) as km:
        assert len(km) == len(keys)
        t = concat_batches(list(pr.builder().with_lookup_columns(km, "fk", lookups()).build()))
        check_probe(t, m, pr.fk)
        # ... and as a set: the same table answers IN SET
        ids = concat_batches(list(pr.builder().with_row_filter(P.in_set("fk", km), prune=False).build())).column("id").to_pylist()
        assert ids == [i for i, k in enumerate(pr.fk) if k in m]


def test_duplicates_are_refused_at_the_seal(tmpdir):
    base = spread(1500, seed=9)
    cases = {"in_one_wavefront": (base[:100], 40, 3, 1), "across_stripes": (base, 1400, 5, 2)}
    for name, (keys, at, of, stripes) in cases.items():
        dup = list(keys)
        dup[at] = keys[of]
        b = Build(tmpdir, "dup_" + name, dup, stripes=stripes)
        with pytest.raises(M.Duplicate):
            b.model()
        with pytest.raises(capi.OrcGpuError) as e:
            b.collect()
        assert e.value.code == UNSUPPORTED and "duplicate key" in str(e.value), name
        # the same data minus the duplicate: accepted
        good = Build(tmpdir, "nodup_" + name, keys, stripes=stripes)
        with good.collect() as km:
            assert len(km) == len(keys)
    # across two readers: the second file repeats one key of the first
    one, two = Build(tmpdir, "dup_r1", base[:70]), Build(tmpdir, "dup_r2", base[69:140])
    km = KeyMap(ctx(), 1 << 10)
    one.collect(into=km)
    two.collect(into=km)
    with pytest.raises(capi.OrcGpuError) as e:
        km.seal()
    assert e.value.code == UNSUPPORTED and "duplicate key" in str(e.value)
    with pytest.raises(capi.OrcGpuError) as e:  # and again: the map stays refused, and no reader probes it
        km.seal()
    assert "duplicate key" in str(e.value)
    km.close()
    two_ok = Build(tmpdir, "dup_r3", base[70:140])
    km = KeyMap(ctx(), 1 << 10)
    one.collect(into=km)
    two_ok.collect(into=km)
    km.seal()
    m = dict(one.model()[0])
    m.update(two_ok.model()[0])
    assert len(km) == 140 and km.rows_seen == 140
    pr = Probe(tmpdir, "p_two_readers", base[:200])
    check_probe(concat_batches(list(pr.builder().with_lookup_columns(km, "fk", lookups()).build())), m, pr.fk)
    km.close()
    # the sentinel's value twice
    b = Build(tmpdir, "dup_sentinel", [1, M.SENTINEL, 2, M.SENTINEL])
    with pytest.raises(capi.OrcGpuError) as e:
        b.collect()
    assert "duplicate key" in str(e.value)
    # a duplicate the row filter does not keep is none
    b = Build(tmpdir, "dup_filtered", [1, 2, 3, 4, 5, 1])
    with b.collect(f_below=5) as km:
        assert len(km) == 5


def test_exactly_max_keys_fits_and_one_more_is_refused(tmpdir):
    b = Build(tmpdir, "b_limit", spread(100, seed=4))
    with b.collect(max_keys=100) as km:
        assert len(km) == 100
    with pytest.raises(capi.OrcGpuError) as e:
        b.collect(max_keys=99)
    assert e.value.code == UNSUPPORTED and "max_keys = 99" in str(e.value)


@pytest.mark.parametrize("bits", ["1", "4"])
def test_a_masked_hash_gives_the_same_answers(tmpdir, side, monkeypatch, bits):
    monkeypatch.setenv("ORCGPU_KEY_SET_HASH_BITS", bits)
    b, p, _ = side
    m, _ = b.model()
    with b.collect(max_keys=128) as km:
        check_probe(concat_batches(list(p.builder().with_lookup_columns(km, "fk", lookups()).build())), m, p.fk)


def lds_limits():
    """the largest max_keys whose sealed table is staged in LDS, from the constant in the code"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orc_rust_amd", "csrc", "device", "filter_program.h")).read()
    lds = int(re.search(r"kInLdsBytes = (\d+);", text).group(1))
    header = int(re.search(r"kInHeaderBytes = (\d+);", text).group(1))

    def table_bytes(max_keys):
        n = 64
        while n < 2 * max_keys:
            n <<= 1
        return header + n // 8 + n * 8

    inside = max(k for k in (1 << s for s in range(1, 20)) if table_bytes(k) <= lds)
    assert table_bytes(inside) <= lds < table_bytes(inside + 1)
    return inside, inside + 1


@pytest.mark.parametrize("which", [0, 1], ids=["lds", "global"])
def test_lds_and_global_probe_paths(tmpdir, which):
    max_keys = lds_limits()[which]
    keys = spread(max_keys, seed=21)
    b = Build(tmpdir, "b_path%d" % which, keys, stripes=(max_keys + 1023) // 1024)
    m, _ = b.model(["v64", "vp"])
    pr = Probe(tmpdir, "p_path%d" % which, [keys[(i * 13) % max_keys] if i % 5 else -i - 10 ** 7 for i in range(1300)], stripes=2)
    with b.collect(["v64", "vp"], max_keys=max_keys) as km:
        assert len(km) == max_keys
        check_probe(concat_batches(list(pr.builder().with_lookup_columns(km, "fk", lookups(["v64", "vp"])).build())), m, pr.fk, ["v64", "vp"])


def test_poison_and_read_ahead(side, monkeypatch):
    monkeypatch.setenv("ORCGPU_POISON", "0xA5")  # a plane entry, a value or a validity word left unwritten shows
    b, p, _ = side
    m, _ = b.model()
    for prefetch in (0, 2):
        with b.collect(prefetch=prefetch) as km:
            check_probe(concat_batches(list(p.builder(prefetch).with_lookup_columns(km, "fk", lookups()).build())), m, p.fk)


def test_two_maps_on_two_keys_and_an_inner_join(tmpdir, side):
    b, p, km = side
    m, _ = b.model()
    b2 = Build(tmpdir, "b_second", list(range(0, 40)), seed=8)
    m2, _ = b2.model(["v8", "vf32"])
    with b2.collect(["v8", "vf32"]) as km2:
        reader = p.builder().with_lookup_columns(km, "fk", {"a": "v32", "b": "vw"}).with_lookup_columns(km2, "c", {"x": "vf32", "y": "v8"}).build()
        t = concat_batches(list(reader))
        assert t.schema.names == ["id", "fk", "fk32", "c", "a", "b", "x", "y"]
        assert got_values(t, "a") == M.probe(m, p.fk, ALL.index("v32")) and got_values(t, "b") == M.probe(m, p.fk, ALL.index("vw"))
        assert got_values(t, "x") == spell("vf32", M.probe(m2, p.c, 1)) and got_values(t, "y") == M.probe(m2, p.c, 0)
    # one map named by a lookup and by in_set: the inner join
    t = concat_batches(list(p.builder().with_lookup_columns(km, "fk", lookups()).with_row_filter(P.in_set("fk", km), prune=False).build()))
    keep = [k in m for k in p.fk]
    assert t.column("id").to_pylist() == [i for i in range(p.n) if keep[i]]
    check_probe(t, m, p.fk, keep=keep)


def test_later_stages_see_a_lookup_column_by_name(tmpdir, side):
    b, p, km = side
    m, _ = b.model()
    v32 = M.probe(m, p.fk, ALL.index("v32"))
    look = p.builder().with_lookup_columns(km, "fk", {"o32": "v32", "op": "vp"})
    # a filter leaf, pruning on and off
    for prune in (True, False):
        t = concat_batches(list(p.builder().with_lookup_columns(km, "fk", {"o32": "v32"}).with_row_filter(P.gt("o32", V.Int64(0)), prune=prune).build()))
        assert t.column("id").to_pylist() == [i for i, v in enumerate(v32) if v is not None and v > 0]
    t = concat_batches(list(p.builder().with_lookup_columns(km, "fk", {"o32": "v32"}).with_row_filter(P.is_null("o32"), prune=False).build()))
    assert t.column("id").to_pylist() == [i for i, v in enumerate(v32) if v is None]
    # collect_keys on it
    with look.collect_keys("o32", max_keys=1 << 12) as ks:
        assert len(ks) == len({v for v in v32 if v is not None}) and ks.has_null
    # collect_map with a lookup column as a value: the two-level chain (probe -> build -> its own values)
    with p.builder().with_lookup_columns(km, "fk", {"o64": "v64", "of": "vf64"}).collect_map("id", ["c", "o64", "of"], max_keys=1 << 12) as chain:
        assert chain.value_types == ["int64", "int64", "float64"] and len(chain) == p.n
        m_chain, _ = M.build(list(range(p.n)), list(zip(p.c, M.probe(m, p.fk, ALL.index("v64")), M.probe(m, p.fk, ALL.index("vf64")))))
        top = Probe(tmpdir, "p_chain", [(i * 37) % (p.n + 50) for i in range(700)])
        t = concat_batches(list(top.builder().with_lookup_columns(chain, "fk", {"c2": "c", "g64": "o64", "gf": "of"}).build()))
        assert got_values(t, "c2") == M.probe(m_chain, top.fk, 0) and got_values(t, "g64") == M.probe(m_chain, top.fk, 1)
        assert got_values(t, "gf") == spell("vf", M.probe(m_chain, top.fk, 2))
    # a computed column over a lookup column stays refused, and says so
    with pytest.raises(capi.OrcGpuError) as e:
        list(p.builder().with_lookup_columns(km, "fk", {"o32": "v32"}).with_computed_columns({"r": col("o32") + 1}).build())
    assert e.value.code == UNSUPPORTED and "'o32' is a lookup column" in str(e.value)
    # beside a computed column over the file's columns: file < lookup < computed
    t = concat_batches(list(p.builder().with_computed_columns({"r": col("c") + 1}).with_lookup_columns(km, "fk", {"o32": "v32"}).build()))
    assert t.schema.names == ["id", "fk", "fk32", "c", "o32", "r"] and got_values(t, "o32") == v32 and got_values(t, "r") == [c + 1 for c in p.c]


def model_aggs(vi, vp, n_rows):
    vi, vp = [v for v in vi if v is not None], [v for v in vp if v is not None]
    avg_p = AEM.avg_decimal(sum(vp), len(vp), 2) if vp else None
    return [n_rows, len(vi), sum(vi) if vi else None, min(vi) if vi else None, max(vi) if vi else None, AEM.avg_int(sum(vi), len(vi)) if vi else None,
            dec(sum(vp), 2) if vp else None, dec(min(vp), 2) if vp else None, dec(max(vp), 2) if vp else None, dec(*avg_p) if vp else None]


AGGS = [Agg.count_rows(), Agg.count("o32"), Agg.sum("o32"), Agg.min("o32"), Agg.max("o32"), Agg.avg("o32"), Agg.sum("op"), Agg.min("op"), Agg.max("op"), Agg.avg("op")]


def test_aggregates_over_lookup_columns(side):
    b, p, km = side
    m, _ = b.model()
    v32, vp, v8 = (M.probe(m, p.fk, ALL.index(v)) for v in ("v32", "vp", "v8"))
    reader = p.builder().with_lookup_columns(km, "fk", {"o32": "v32", "op": "vp"}).aggregating_reader(AGGS)
    assert reader.aggregate() == model_aggs(v32, vp, p.n)
    assert reader.d2h_bytes() == 0
    # GROUP BY a looked-up Int64 and a Decimal key, on the hashed path and the wide one
    for key, keys in (("o8", v8), ("op", vp)):
        groups = {}
        for i, v in enumerate(keys):
            groups.setdefault(v, []).append(i)
        for limit in (None, 1024):
            res = p.builder().with_lookup_columns(km, "fk", {"o32": "v32", "op": "vp", "o8": "v8"}).aggregate(AGGS, group_by=[key], max_groups=limit)
            assert [k[0] for k, _ in res] == [None if v is None else v if key == "o8" else dec(v, 2) for v in groups], (key, limit)
            for (k, got), idx in zip(res, groups.values()):
                assert got == model_aggs([v32[i] for i in idx], [vp[i] for i in idx], len(idx)), (key, limit, k)
    with pytest.raises(capi.OrcGpuError) as e:  # a Float64 key stays refused
        p.builder().with_lookup_columns(km, "fk", {"of": "vf64"}).aggregate([Agg.count_rows()], group_by=["of"])
    assert "of" in str(e.value)


def test_top_k_by_a_lookup_column(side):
    b, p, km = side
    look = {"o32": "v32", "op": "vp"}
    full = concat_batches(list(p.builder().with_lookup_columns(km, "fk", look).build()))
    for key, desc, nf in (("o32", False, False), ("op", True, True)):
        got = p.builder().with_lookup_columns(km, "fk", look).top_k([SortKey(key, descending=desc, nulls_first=nf), SortKey("id")], 50)
        want, _ = TK.top_k_table(full, [(key, desc, nf), ("id", False, False)], 50)
        assert got.schema.names == want.schema.names and got.num_rows == 50
        for name in want.schema.names:
            assert got_values(got, name) == got_values(want, name), (key, name)


def test_selection_and_row_filter(side):
    b, p, km = side
    m, _ = b.model()
    sel = [(100, True), (30, False), (900, True), (70, False), (600, True), (349, False)]  # (to the file's end)
    picked = np.zeros(p.n, bool)
    at = 0
    for count, skip in sel:
        if not skip:
            picked[at:at + count] = True
        at += count
    assert at == p.n
    kept_f = np.array([c < 5 for c in p.c])
    for use_sel, use_filter in ((True, False), (False, True), (True, True)):
        for prune in (True, False):
            bd = p.builder().with_lookup_columns(km, "fk", lookups()).with_row_group_pruning(prune)
            keep = np.ones(p.n, bool)
            if use_sel:
                bd = bd.with_row_selection(sel)
                keep &= picked
            if use_filter:
                bd = bd.with_row_filter(P.lt("c", V.Int64(5)), prune=prune)
                keep &= kept_f
            t = concat_batches(list(bd.build()))
            assert t.column("id").to_pylist() == [i for i in range(p.n) if keep[i]]
            check_probe(t, m, p.fk, keep=list(keep))


def test_device_output_equals_the_host_path(side):
    b, p, km = side
    host = concat_batches(list(p.builder().with_lookup_columns(km, "fk", lookups()).build()))
    reader = p.builder().with_lookup_columns(km, "fk", lookups()).with_device_output().build()
    dev = [bt.to_pyarrow() for bt in reader]
    assert reader.d2h_bytes() == 0
    table = concat_batches(dev)
    assert table.schema.names == host.schema.names
    for v in ALL:
        assert got_values(table, "o_" + v) == got_values(host, "o_" + v), v


def test_the_build_copies_nothing_back(side):
    b, _, _ = side
    reader = b.builder().build()
    km = KeyMap(ctx(), 1 << 8)
    reader.collect_map("k", ALL, km)
    assert reader.d2h_bytes() == 0
    reader.close()
    km.seal()
    assert len(km) == 65
    km.close()


def test_result_level_entry_points_on_a_hand_decoded_result():
    c = TA.ctx()
    n = 2 * 1000 + 65
    res, table = TA.stripe_result(n, 1000)
    ids, v = table.column("id").to_pylist(), table.column("v").to_pylist()
    kept = [i % 3 == 0 for i in ids]
    km = KeyMap(c, 1 << 12)
    c.result_collect_map(res, "id", ["v"], km, ["id", "v"], predicate=P.in_list("id", [V.Int64(i) for i in ids if i % 3 == 0]))
    km.seal()
    m, _ = M.build(ids, [(x,) for x in v], kept)
    assert len(km) == len(m) and km.value_types == ["int64"] and km.rows_seen == n
    res.free()
    res, _ = TA.stripe_result(n, 1000)
    c.result_lookup_columns(res, km, "id", {"back": "v"}, ["id", "v"])

    def column(res, colm):
        out = []
        for bt in range(res.n_batches):
            x = res.batch(bt, colm)
            vals = np.frombuffer(x["values"], dtype=np.int64)[:x["length"]]
            valid = np.unpackbits(np.frombuffer(x["validity"], dtype=np.uint8), bitorder="little")[:x["length"]] if x["validity"] is not None else np.ones(x["length"], np.uint8)
            assert x["null_count"] == int((valid == 0).sum())
            out += [int(a) if ok else None for a, ok in zip(vals, valid)]
        return out

    assert column(res, 0) == ids and column(res, 1) == v  # the decode's own columns are where they were
    assert column(res, 2) == M.probe(m, ids, 0)
    with pytest.raises(capi.OrcGpuError) as e:
        c.result_lookup_columns(res, km, "id", {"again": "v"}, ["id", "v", "back"])
    assert e.value.code == INVALID and "already holds" in str(e.value)
    res.free()
    km.close()


def test_closing_the_map_under_a_live_reader(side):
    b, p, _ = side
    m, _ = b.model(["v64"])
    km = b.collect(["v64"])
    reader = p.builder().with_lookup_columns(km, "fk", {"x": "v64"}).build()
    first = next(iter(reader))
    km.close()
    rest = list(reader)
    t = concat_batches([first] + rest)
    assert got_values(t, "x") == M.probe(m, p.fk, 0)


def test_c_side_refusals(tmpdir, side):
    b, p, km = side
    strings = str(tmpdir / "kinds.orc")
    orc.write_table(pa.table({"k": pa.array([1, 2, 3], pa.int64()), "s": pa.array(["a", "b", "c"]), "t": pa.array([True, False, None]),
                              "ts": pa.array([1, 2, 3], pa.timestamp("us")), "st": pa.array([{"f": 1}, {"f": 2}, None], pa.struct([("f", pa.int64())]))}), strings)

    def collect_refused(key, values, code, words, projection=("k", "s", "t", "ts"), dictionary=None, path=strings):
        bd = ArrowReaderBuilder.try_new(path, ctx()).with_prefetch(0)
        if projection:
            bd = bd.with_projection(list(projection))
        if dictionary:
            bd = bd.with_dictionary_columns(dictionary)
        with pytest.raises(capi.OrcGpuError) as e:
            bd.collect_map(key, values)
        assert e.value.code == code and words in str(e.value), str(e.value)

    collect_refused("k", ["s"], UNSUPPORTED, "value column 's' is a String")
    collect_refused("k", ["t"], UNSUPPORTED, "value column 't' is a Boolean")
    collect_refused("k", ["ts"], UNSUPPORTED, "value column 'ts' is a Timestamp")
    collect_refused("k", ["s"], UNSUPPORTED, "value column 's'", dictionary=["s"])
    collect_refused("k", ["st"], UNSUPPORTED, "st", projection=("k", "st"))
    collect_refused("k", ["nope"], INVALID, "value column 'nope' is not a projected root column")
    collect_refused("k", ["ts"], INVALID, "value column 'ts' is not a projected root column", projection=("k", "s"))
    collect_refused("nope", ["k"], INVALID, "column 'nope' is not a projected root column")
    collect_refused("s", ["k"], UNSUPPORTED, "column 's' is a String")
    # a later collect whose values differ from the first's
    open_map = KeyMap(ctx(), 1 << 8)
    b.collect(["v64"], into=open_map)
    open_map.value_names = None  # (past the Python check: the library's own refusal)
    with pytest.raises(capi.OrcGpuError) as e:
        b.collect(["vp"], into=open_map)
    assert e.value.code == MISMATCHED and "differ from those of the map's first collect" in str(e.value)
    # an unsealed map cannot be probed (past the Python check)
    open_map._info = capi.KeyMapInfo()
    open_map.value_names = ["v64"]
    with pytest.raises(capi.OrcGpuError) as e:
        p.builder().with_lookup_columns(open_map, "fk", {"x": "v64"})
    assert e.value.code == INVALID and "not sealed yet" in str(e.value)
    open_map.close()

    def lookup_refused(key, columns, code, words, path=None, projection=None, first=None):
        bd = ArrowReaderBuilder.try_new(path or p.path, ctx()).with_prefetch(0)
        if projection:
            bd = bd.with_projection(projection)
        with pytest.raises(capi.OrcGpuError) as e:
            if first:
                bd = first(bd)
            list(bd.with_lookup_columns(km, key, columns).build())
        assert e.value.code == code and words in str(e.value), str(e.value)

    lookup_refused("fk", {"c": "v64"}, INVALID, "'c' is the name of a root column of the file")
    lookup_refused("fk", {"c": "v64"}, INVALID, "'c' is the name of a root column of the file", projection=["id", "fk"])
    lookup_refused("nope", {"x": "v64"}, INVALID, "its probe key 'nope' is not a projected root column")
    lookup_refused("c", {"x": "v64"}, INVALID, "its probe key 'c' is not a projected root column", projection=["id", "fk"])
    lookup_refused("s", {"x": "v64"}, UNSUPPORTED, "column 's' is a String", path=strings, projection=["k", "s"])
    lookup_refused("k", {"x": "v64"}, UNSUPPORTED, "the projected column 'st' is nested", path=strings)
    lookup_refused("fk", {"r": "v64"}, INVALID, "'r' is the name of a computed column", first=lambda bd: bd.with_computed_columns({"r": col("c") + 1}))
    lookup_refused("r", {"x": "v64"}, UNSUPPORTED, "its probe key 'r' is a computed column", first=lambda bd: bd.with_computed_columns({"r": col("c") + 1}))
    # a map of another context
    other = capi.Context()
    with pytest.raises(ValueError, match="another context"):
        ArrowReaderBuilder.try_new(p.path, other).with_lookup_columns(km, "fk", {"x": "v64"})
    spec = (capi.LookupSpec * 1)()
    spec[0].name, spec[0].key_column, spec[0].map, spec[0].value = b"x", b"fk", km._h, 0
    bd = ArrowReaderBuilder.try_new(p.path, other)
    assert other.L.orcgpu_reader_set_lookup_columns(bd._h, spec, 1) == INVALID
    spec[0].value = 8  # a value index past the map's values
    bd = ArrowReaderBuilder.try_new(p.path, ctx())
    assert ctx().L.orcgpu_reader_set_lookup_columns(bd._h, spec, 1) == INVALID
    # set after the reader has been built
    bd = ArrowReaderBuilder.try_new(p.path, ctx()).with_prefetch(0)
    assert ctx().L.orcgpu_reader_column_count(bd._h) == 4
    with pytest.raises(capi.OrcGpuError) as e:
        bd.with_lookup_columns(km, "fk", {"x": "v64"})
    assert e.value.code == INVALID and "after the reader has been built" in str(e.value)


def test_without_lookup_columns_nothing_changes(side):
    """a reader that is given no lookup columns hands out what pyarrow reads of the file, host and device output alike"""
    _, p, _ = side
    batches = list(p.builder().build())
    assert all(bt.schema.names == ["id", "fk", "fk32", "c"] for bt in batches)
    ours, theirs = concat_batches(batches), orc.ORCFile(p.path).read()
    dev = concat_batches([bt.to_pyarrow() for bt in p.builder().with_device_output().build()])
    for name in ("id", "fk", "fk32", "c"):
        assert ours.column(name).to_pylist() == theirs.column(name).to_pylist() == dev.column(name).to_pylist(), name
