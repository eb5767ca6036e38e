#!/usr/bin/env python3
"""What a lookup join costs the file reader, against joining on the host.

The lineitem file of profiles/reader_filter.py (ORC C++ writer, Zstandard, 64 MiB stripes) and an orders-shaped build side made
from it: one row per distinct l_orderkey with o_orderdate (Date) and o_shippriority (Int), written as a second ORC file.  Q3-shaped:
lineitem grouped by the two looked-up columns, SUM(l_extendedprice) and COUNT(*).  One process, a warm-up and best of three per arm,
every pass listed with the spread:
  build    orders -> collect_map(o_orderkey, [o_orderdate, o_shippriority]): key_map_insert_kernel per stripe, one seal
  probe    lineitem with two lookup columns (ONE probe per row, lookup_columns_kernel; the decode call on one column lane),
           aggregated on the GPU, wide GROUP BY path; d2h_bytes must stay 0
  plain    the same probing read -- l_orderkey and l_extendedprice -- aggregated without the lookup: what the reader costs alone
  host     both tables read back, pyarrow.Table.join and group_by on the same box
`probe` and `host` are held to the same groups and values.  A kernel trace of one build + probe pass in a child process of its own
under rocprofv3 --kernel-trace --stats gives the two new kernels' shares (left out where rocprofv3 is not there).
No mark is set in advance: nobody has measured a per-row gather from value planes of hundreds of MiB.
    python3 profiles/reader_lookup_join.py [rows] [out.json]      writes profiles/reader_lookup_join.json"""
import csv, glob, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
if not os.path.isdir("/usr/share/zoneinfo"):
    import tzdata; os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.orc as orc
import torch  # noqa: F401
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg
from orc_rust_amd.arrow_reader import ArrowReaderBuilder, concat_batches
LOOK = {"o_orderdate": "o_orderdate", "o_shippriority": "o_shippriority"}
SPECS = [Agg.sum("l_extendedprice"), Agg.count_rows()]
def builder(ctx, path, cols):
    return ArrowReaderBuilder.try_new(path, ctx).with_batch_size(65536).with_prefetch(2).with_projection(cols)
def build(ctx, orders, max_keys):
    t0 = time.perf_counter()
    km = builder(ctx, orders, ["o_orderkey", "o_orderdate", "o_shippriority"]).collect_map("o_orderkey", list(LOOK.values()), max_keys=max_keys)
    return time.perf_counter() - t0, km
def probe(ctx, lineitem, km, n_groups):
    t0 = time.perf_counter()
    r = builder(ctx, lineitem, ["l_orderkey", "l_extendedprice"]).with_lookup_columns(km, "l_orderkey", LOOK).aggregating_reader(
        SPECS, group_by=["o_orderdate", "o_shippriority"], max_groups=n_groups, max_total_groups=n_groups)
    groups = r.aggregate()
    assert r.d2h_bytes() == 0
    return time.perf_counter() - t0, sorted((k, tuple(v)) for k, v in groups)
def plain(ctx, lineitem):
    t0 = time.perf_counter()
    got = builder(ctx, lineitem, ["l_orderkey", "l_extendedprice"]).aggregate(SPECS)
    return time.perf_counter() - t0, got
def host(ctx, lineitem, orders):
    t0 = time.perf_counter()
    li = concat_batches(list(builder(ctx, lineitem, ["l_orderkey", "l_extendedprice"]).build()))
    od = concat_batches(list(builder(ctx, orders, ["o_orderkey", "o_orderdate", "o_shippriority"]).build()))
    j = li.join(od, keys="l_orderkey", right_keys="o_orderkey", join_type="left outer")
    g = j.group_by(["o_orderdate", "o_shippriority"]).aggregate([("l_extendedprice", "sum"), ([], "count_all")])
    rows = sorted(((d, p), (s, c)) for d, p, s, c in zip(g.column("o_orderdate").to_pylist(), g.column("o_shippriority").to_pylist(),
                                                        g.column("l_extendedprice_sum").to_pylist(), g.column("count_all").to_pylist()))
    return time.perf_counter() - t0, rows
if len(sys.argv) > 3 and sys.argv[1] == "--one-pass":  # the child under rocprofv3: one build and one probe
    c = capi.Context(0)
    _, m = build(c, sys.argv[3], int(sys.argv[4]))
    probe(c, sys.argv[2], m, int(sys.argv[5]))
    sys.exit(0)
import make_lineitem
from orc_rust_amd.gen import workloads as W
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 24_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "reader_lookup_join.json")
tmp = tempfile.mkdtemp()
lineitem, orders = os.path.join(tmp, "li.orc"), os.path.join(tmp, "orders.orc")
li_table = make_lineitem.arrow_table(W.lineitem_table(rows), rows)
orc.write_table(li_table, lineitem, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
keys = pc.unique(li_table.column("l_orderkey")).to_numpy()
rng = np.random.default_rng(1)
n_dates = 2406  # the days of 1992-01-01 .. 1998-08-02
orc.write_table(pa.table({"o_orderkey": pa.array(keys, pa.int64()), "o_orderdate": pa.array(8035 + rng.integers(0, n_dates, len(keys)), pa.int32()).cast(pa.date32()),
                          "o_shippriority": pa.array(rng.integers(0, 2, len(keys)), pa.int32())}), orders, compression="zstd", stripe_size=64 << 20)
del li_table
max_keys, n_groups = len(keys), 2 * n_dates + 16
ctx = capi.Context(0)
out = {"lineitem": {"rows": rows, "bytes": os.path.getsize(lineitem)}, "orders": {"rows": len(keys), "bytes": os.path.getsize(orders)}, "batch_size": 65536, "prefetch": 2,
       "warmup": 1, "repeats": 3}
def spread(ms):
    return {"ms_best": round(min(ms), 1), "ms_all": [round(m, 1) for m in ms], "spread": round((max(ms) - min(ms)) / min(ms), 4)}
build_ms, probe_ms, got = [], [], None
for k in range(4):  # (the first pass warms up)
    tb, km = build(ctx, orders, max_keys)
    tp, got = probe(ctx, lineitem, km, n_groups)
    km.close()
    if k:
        build_ms.append(tb * 1e3), probe_ms.append(tp * 1e3)
out["build"], out["probe"] = spread(build_ms), spread(probe_ms)
plain(ctx, lineitem)
out["plain"] = spread([plain(ctx, lineitem)[0] * 1e3 for _ in range(3)])
host(ctx, lineitem, orders)
passes = [host(ctx, lineitem, orders) for _ in range(3)]
out["host"] = spread([p[0] * 1e3 for p in passes])
want = passes[0][1]
assert [(k, (s, c)) for k, (s, c) in got] == [((d, p), (s, c)) for (d, p), (s, c) in want], "the lookup join and the host join give different groups or values"
out["groups"], out["values_agree"] = len(got), True
out["build_plus_probe_over_host"] = round((out["build"]["ms_best"] + out["probe"]["ms_best"]) / out["host"]["ms_best"], 3)
out["probe_over_plain"] = round(out["probe"]["ms_best"] / out["plain"]["ms_best"], 3)
print(json.dumps(out))
if shutil.which("rocprofv3"):
    prof = os.path.join(tmp, "prof")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "lookup", "--", sys.executable, os.path.abspath(__file__), "--one-pass", lineitem, orders,
                    str(max_keys), str(n_groups)], check=False, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    total, mine = 0.0, {"key_map_insert_kernel": 0.0, "lookup_columns_kernel": 0.0}
    for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            ns = float(row.get("TotalDurationNs", 0) or 0)
            total += ns
            for name in mine:
                if name in row.get("Name", ""):
                    mine[name] += ns
    if total:
        out["kernel_trace"] = {"device_ms": round(total / 1e6, 1), **{k + "_ms": round(v / 1e6, 2) for k, v in mine.items()}, **{k + "_share": round(v / total, 5) for k, v in mine.items()}}
json.dump(out, open(out_path, "w"), indent=1)
shutil.rmtree(tmp, ignore_errors=True)
