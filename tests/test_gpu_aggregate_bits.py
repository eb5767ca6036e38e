"""The aggregates' records bit for bit: the order in which the kernels of device/agg_kernels.hip and device/agg_group_kernels.hip
fold Float sums is a contract (the same call gives the same bits, from one commit to the next), and the other GPU tests judge a
Float sum by a bound only.  tests/golden/aggregate_bits.json holds the raw orcgpu_agg_value records of the commit it names, per size,
arm and grouping: the keys of the groups in the order handed out, and the groups' records in that order, ten of 48 bytes a group, as
one run of bytes -- deflated (zlib) and then written as hex, which keeps six thousand records at a size that can be read past.  A
test asserts byte equality of the records with the inflated run (a difference is reported by group and aggregate, both sides as
hex) and, so that the golden is not the only judge, that the exact kinds (counts, SUM of an Int64 column, MIN / MAX) equal what
numpy computes from the arrays the file was generated from.

The inputs are integer formulas of the row number, never a random generator's: the same everywhere.  One row in five is NULL in
each of the aggregated columns (i, fa, fb, g); `id` and the filter's column `m` hold every row, so that `m <> 0` keeps a scattered
two thirds.  The two Float64 columns span twelve decades, so that a change of the order of summation shows in the low bits.

Sizes, and what each reaches: 65 a tail word; 1025 several blocks; 2049 in two stripes the merge of stripes in the reader; 33 000
a second trip of a wavefront in agg_group_partial_body (agg_group_blocks stops at 128 blocks: 32 768 rows a trip); 262 209 a second
trip in agg_partial_body (agg_blocks stops at 1024 blocks: 262 144 rows a trip) -- ungrouped and k4 only.

Recording the golden (in a checkout of the commit to record, with this file copied in; on a machine with the GPU):
    cd tests && python -m test_gpu_aggregate_bits <commit hash> [<output path>]"""
import json
import os
import re
import sys
import zlib

import numpy as np
import pyarrow as pa
import pytest
import torch  # noqa: F401  (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (python -m from tests/ runs without the conftest)
    sys.path.insert(0, ROOT)

import test_gpu_aggregate as TA  # noqa: E402
from orc_rust_amd.aggregate import Agg, col, lit  # noqa: E402
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "aggregate_bits.json")
NAMES = ["id", "m", "i", "fa", "fb", "g", "k4", "k64"]
# (rows, stripes, groupings): "" is the ungrouped call
CASES = ((65, 1, ("", "k4", "k64")), (1025, 1, ("", "k4", "k64")), (2049, 2, ("", "k4", "k64")), (33_000, 1, ("", "k4", "k64")), (262_209, 1, ("", "k4")))
ARMS = (("none", None), ("two_thirds", P.ne("m", V.Int64(0))))
SPECS = [Agg.count_rows(), Agg.count("i"), Agg.sum("i"), Agg.sum("fa"), Agg.sum("g"), Agg.sum_product("fa", "fb"), Agg.min("fa"), Agg.max("fa"),
         Agg.sum(col("fa") * lit(1.5) + col("fb")), Agg.avg("fa")]
# ten to the -6 .. 6, as the literals a compiler rounds correctly: twelve decades
DECADES = np.array([1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6])
_GOLDEN = None


def columns(n):
    """name -> (values, null mask or None), every value an integer formula of the row number"""
    r = np.arange(n, dtype=np.int64)
    sign = 1 - 2 * (r % 2)
    return {
        "id": (r, None),
        "m": (r % 3, None),
        "i": ((r * 2654435761) % (1 << 40) - (1 << 39), r % 5 == 0),
        "fa": ((sign * ((r * 37) % 1000 + 1)).astype(np.float64) * DECADES[(r * 5) % 13], r % 5 == 1),
        "fb": (((r * 53) % 2001 - 1000).astype(np.float64) * DECADES[(r * 7 + 3) % 13], r % 5 == 2),
        "g": ((((r * 11) % 2001 - 1000).astype(np.float64) / 8).astype(np.float32), r % 5 == 3),
        "k4": ((7 * r) % 4, None),
        "k64": ((5 * r) % 64, None),
    }


def make_file(n, stripes):
    cols = columns(n)
    table = pa.table({name: pa.array(v, mask=mask) for name, (v, mask) in cols.items()})
    return cols, TA.own_file(table, stripes=stripes)[0]


def records(data, pred, grouping):
    """The raw records: ungrouped [hex per spec]; grouped [[key, [hex per spec]] per group, in the order handed out]"""
    r = TA.builder(data, NAMES, pred=pred).aggregating_reader(SPECS, group_by=[grouping] if grouping else None)
    try:
        raw = r.aggregate(raw=True)
        assert r.d2h_bytes() == 0
    finally:
        r.close()
    if not grouping:
        return [bytes(v).hex() for v in raw]
    return [[int(keys[0]), [bytes(v).hex() for v in vals]] for keys, vals in raw]


def exact(hexes, cols, keep, what):
    """counts, SUM(i), MIN / MAX(fa) of the kept rows against numpy"""
    from orc_rust_amd import aggregate as A
    vals = [A.AggValue.from_buffer_copy(bytes.fromhex(h)) for h in hexes]
    i, i_null = cols["i"]
    fa, fa_null = cols["fa"]
    got = [A.value_of(vals[k], SPECS[k]) for k in (0, 1, 2, 6, 7)]
    ki, kf = keep & ~i_null, keep & ~fa_null
    want = [int(keep.sum()), int(ki.sum()), int(i[ki].sum()) if ki.any() else None, float(fa[kf].min()) if kf.any() else None,
            float(fa[kf].max()) if kf.any() else None]
    assert got == want, (what, got, want)


def exact_all(recs, cols, keep, grouping, what):
    if not grouping:
        return exact(recs, cols, keep, what)
    key = cols[grouping][0]
    kept_keys, first = np.unique(key[keep], return_index=True)
    assert [k for k, _ in recs] == [int(k) for k in kept_keys[np.argsort(first)]], what      # the order handed out: first appearance
    for k, hexes in recs:
        exact(hexes, cols, keep & (key == k), (what, k))


def pack(recs, grouping):
    """records() -> what the golden holds of it: {"keys": [key per group], "deflate_hex": the records' bytes, deflated, as hex}"""
    groups = recs if grouping else [[None, recs]]
    raw = b"".join(bytes.fromhex(h) for _, hexes in groups for h in hexes)
    return {"keys": [k for k, _ in groups if grouping], "deflate_hex": zlib.compress(raw, 9).hex()}


def assert_same_bytes(recs, grouping, want, what):
    got = pack(recs, grouping)
    assert got["keys"] == want["keys"], (what, got["keys"], want["keys"])
    raw_got, raw_want = zlib.decompress(bytes.fromhex(got["deflate_hex"])), zlib.decompress(bytes.fromhex(want["deflate_hex"]))
    n_groups = len(got["keys"]) if grouping else 1
    assert len(raw_got) == len(raw_want) == 48 * len(SPECS) * n_groups, (what, len(raw_got), len(raw_want))
    for k in range(0, len(raw_want), 48):
        g, spec = divmod(k // 48, len(SPECS))
        assert raw_got[k:k + 48] == raw_want[k:k + 48], (what, "group %d" % g, SPECS[spec], raw_got[k:k + 48].hex(), raw_want[k:k + 48].hex())


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with open(GOLDEN) as f:
            _GOLDEN = json.load(f)
    return _GOLDEN


@pytest.mark.parametrize("n,stripes,groupings", CASES, ids=[str(c[0]) for c in CASES])
def test_records_are_the_recorded_bits(n, stripes, groupings):
    cols, data = make_file(n, stripes)
    want = golden()["records"][str(n)]
    for arm, pred in ARMS:
        keep = np.ones(n, bool) if pred is None else cols["m"][0] != 0
        for grouping in groupings:
            got = records(data, pred, grouping)
            exact_all(got, cols, keep, grouping, (n, arm, grouping))
            assert_same_bytes(got, grouping, want[arm][grouping], (n, arm, grouping, "against the records of commit %s" % golden()["commit"]))


def record(commit, path=GOLDEN):
    out = {"commit": commit, "records": {}}
    for n, stripes, groupings in CASES:
        _, data = make_file(n, stripes)
        out["records"][str(n)] = {arm: {g: pack(records(data, pred, g), g) for g in groupings} for arm, pred in ARMS}
    text = re.sub(r"\[\s+([\d,\s]+?)\s+\]", lambda m: "[" + " ".join(m.group(1).split()) + "]", json.dumps(out, indent=1))   # (a key list on one line)
    with open(path, "w") as f:
        f.write(text + "\n")
    print("recorded", path)


if __name__ == "__main__":
    record(*sys.argv[1:3])
