#!/usr/bin/env python3
"""What a semi-join through a key set costs the file reader, against the only route to the same rows without it.

Probe side: the lineitem file of profiles/reader_filter.py (ORC C++ writer, Zstandard, 64 MiB stripes), l_orderkey and
l_extendedprice read.  Build side: a table written with pyarrow.orc from the file's distinct l_orderkey plus a random date
(o_orderkey, o_orderdate); a filter o_orderdate < X keeps about 1 %, 10 % and 50 % of its keys.  Per share, in one process, best of
three with every pass listed:
  set    build = collect_keys + seal (the build side read, filtered and hashed on the GPU), probe = the lineitem read under
         Predicate.in_set
  host   build = the build side read under the same filter and its keys brought to the host; probe = Predicate.in_list where the
         keys fit ORCGPU_IN_MAX_VALUES (65536), otherwise a full read plus pyarrow.compute.is_in on the host
Both arms must keep the same row count.  The shares of key_set_insert_kernel and filter_in_kernel of the device time come from a
pass of the set arm in a child process of its own under rocprofv3 --kernel-trace --stats (left out where rocprofv3 is not there).
    python3 profiles/reader_semi_join.py [rows] [out.json]      writes profiles/reader_semi_join.json"""
import csv, glob, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
if not os.path.isdir("/usr/share/zoneinfo"):
    import tzdata; os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.orc as orc
from orc_rust_amd import capi
from orc_rust_amd.arrow_reader import ArrowReaderBuilder, concat_batches
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
IN_MAX = 65536
PROBE_COLS = ["l_orderkey", "l_extendedprice"]
def build_builder(ctx, orders, before):
    return (ArrowReaderBuilder.try_new(orders, ctx).with_batch_size(65536).with_prefetch(2).with_projection(["o_orderkey", "o_orderdate"])
            .with_row_filter(P.lt("o_orderdate", V.Int32(before)), prune=False))
def probe_rows(ctx, lineitem, pred):
    b = ArrowReaderBuilder.try_new(lineitem, ctx).with_batch_size(65536).with_prefetch(2).with_projection(PROBE_COLS)
    r = (b.with_row_filter(pred, prune=False) if pred is not None else b).build()
    batches = list(r)
    r.close()
    return batches
def set_arm(ctx, orders, lineitem, before, max_keys):
    t0 = time.perf_counter()
    keys = build_builder(ctx, orders, before).collect_keys("o_orderkey", max_keys=max_keys)
    t1 = time.perf_counter()
    n = sum(b.num_rows for b in probe_rows(ctx, lineitem, P.in_set("l_orderkey", keys)))
    t2 = time.perf_counter()
    n_keys = len(keys)
    keys.close()
    return t1 - t0, t2 - t1, n, n_keys
def host_arm(ctx, orders, lineitem, before):
    t0 = time.perf_counter()
    batches = list(build_builder(ctx, orders, before).build())
    keys = concat_batches(batches).column("o_orderkey").combine_chunks() if batches else pa.array([], pa.int64())
    t1 = time.perf_counter()
    if len(keys) <= IN_MAX:
        route = "in_list"
        n = sum(b.num_rows for b in probe_rows(ctx, lineitem, P.in_list("l_orderkey", [V.Int64(k) for k in keys.to_pylist()])))
    else:
        route = "full read + pyarrow.compute.is_in"
        n = sum(int(pc.sum(pc.is_in(b.column("l_orderkey"), value_set=keys)).as_py() or 0) for b in probe_rows(ctx, lineitem, None))
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, n, len(keys), route
if len(sys.argv) > 2 and sys.argv[1] == "--one-pass":  # the child under rocprofv3: the set arm, one pass
    set_arm(capi.Context(0), sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]))
    sys.exit(0)
import make_lineitem
from orc_rust_amd.gen import workloads as W
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 24_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "reader_semi_join.json")
tmp = tempfile.mkdtemp()
lineitem, orders = os.path.join(tmp, "li.orc"), os.path.join(tmp, "orders.orc")
table = make_lineitem.arrow_table(W.lineitem_table(rows), rows)
orc.write_table(table, lineitem, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
okeys = np.unique(table.column("l_orderkey").to_numpy())
del table
dates = np.random.default_rng(1).integers(0, 10_000, len(okeys)).astype(np.int32)
orc.write_table(pa.table({"o_orderkey": pa.array(okeys), "o_orderdate": pa.array(dates).cast(pa.date32())}), orders, compression="zstd", stripe_size=64 << 20)
max_keys = 1
while max_keys < len(okeys):
    max_keys <<= 1
ctx = capi.Context(0)
out = {"file": {"rows": rows, "bytes": os.path.getsize(lineitem), "build_rows": int(len(okeys)), "build_bytes": os.path.getsize(orders)},
       "max_keys": max_keys, "batch_size": 65536, "prefetch": 2, "warmup": 1, "repeats": 3, "runs": []}
def spread(ms):
    return round((max(ms) - min(ms)) / min(ms), 4)
for share in (0.01, 0.10, 0.50):
    before = int(10_000 * share)
    set_arm(ctx, orders, lineitem, before, max_keys)
    s = [set_arm(ctx, orders, lineitem, before, max_keys) for _ in range(3)]
    host_arm(ctx, orders, lineitem, before)
    h = [host_arm(ctx, orders, lineitem, before) for _ in range(3)]
    assert s[0][2] == h[0][2], ("the two arms keep different row counts", share, s[0][2], h[0][2])
    assert s[0][3] == h[0][3] == int((dates < before).sum())
    run = {"share": share, "keys": s[0][3], "rows_kept": s[0][2], "rows_agree": True, "host_route": h[0][4]}
    for arm, passes in (("set", s), ("host", h)):
        for part, k in (("build", 0), ("probe", 1)):
            ms = [p[k] * 1e3 for p in passes]
            run["%s_%s_ms_best" % (arm, part)], run["%s_%s_ms_all" % (arm, part)], run["%s_%s_spread" % (arm, part)] = round(min(ms), 1), [round(m, 1) for m in ms], spread(ms)
    run["set_over_host_total"] = round((run["set_build_ms_best"] + run["set_probe_ms_best"]) / (run["host_build_ms_best"] + run["host_probe_ms_best"]), 3)
    out["runs"].append(run)
    print(json.dumps(run))
if shutil.which("rocprofv3"):
    prof = os.path.join(tmp, "prof")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "semi", "--", sys.executable, os.path.abspath(__file__), "--one-pass", orders, lineitem, "1000",
                    str(max_keys)], check=False, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    total, mine = 0.0, {"key_set_insert_kernel": 0.0, "key_set_seal_kernel": 0.0, "filter_in_kernel": 0.0}
    for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            ns = float(row.get("TotalDurationNs", 0) or 0)
            total += ns
            for k in mine:
                if row.get("Name", "").startswith(k):
                    mine[k] += ns
    if total:
        out["kernel_trace"] = {"share_kept": 0.10, "device_ms": round(total / 1e6, 1), **{k + "_share": round(v / total, 5) for k, v in mine.items()}}
json.dump(out, open(out_path, "w"), indent=1)
shutil.rmtree(tmp, ignore_errors=True)
