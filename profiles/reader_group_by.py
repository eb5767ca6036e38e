#!/usr/bin/env python3
"""What the GROUP BY of TPC-H Q1 costs the file reader, in one process: the lineitem file of profiles/reader_aggregate.py (ORC C++
writer, Zstandard, 64 MiB stripes), every arm on the projection l_returnflag, l_linestatus (plain Utf8 reads), l_quantity,
l_extendedprice, l_discount (Decimal(15, 2)); the aggregates count(*), sum(l_quantity), sum(l_extendedprice), sum(l_discount),
sum(l_extendedprice * l_discount), grouped by l_returnflag, l_linestatus:
  (a) host_group_by        the unfiltered host read, then pyarrow.Table.group_by(...).aggregate(...)
  (b) aggregate_groups     aggregate(specs, group_by=keys)
  (c) aggregate_ungrouped  aggregate(specs), no group_by: the price of grouping is (b) - (c)
  (d) the same two under a row filter on l_quantity: host_group_by_filter, aggregate_groups_filter
One warm-up pass per arm, then the best of three with each arm's spread.  (a) and (b) -- and the two of (d) -- must return the
same groups and the same Decimals: asserted.  The kernels' shares of the device time come from a pass of (b) in a child process of
its own under rocprofv3 --kernel-trace --stats, a run with no counters alongside (left out where rocprofv3 is not there).
    python3 profiles/reader_group_by.py [rows] [out.json]      writes profiles/reader_group_by.json"""
import csv, glob, json, os, shutil, subprocess, sys, tempfile, time
from decimal import Decimal as D
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
if not os.path.isdir("/usr/share/zoneinfo"):
    import tzdata; os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
import torch
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
KEYS = ["l_returnflag", "l_linestatus"]
VALUES = ["l_quantity", "l_extendedprice", "l_discount"]
NAMES = KEYS + VALUES
FILTER = P.lt("l_quantity", V.Decimal128(D("24")))
SPECS = [Agg.count_rows(), Agg.sum("l_quantity"), Agg.sum("l_extendedprice"), Agg.sum("l_discount"), Agg.sum_product("l_extendedprice", "l_discount")]
def builder(ctx, path, pred):
    b = ArrowReaderBuilder.try_new(path, ctx).with_batch_size(65536).with_prefetch(2).with_projection(NAMES)
    return b.with_row_filter(pred, prune=False) if pred is not None else b
def one_pass(ctx, path, arm):
    """(seconds, the arm's answer as a sorted list of (keys, values), bytes copied back)"""
    import pyarrow as pa, pyarrow.compute as pc
    pred = FILTER if arm.endswith("_filter") else None
    t0 = time.perf_counter()
    if arm.startswith("aggregate_groups"):
        r = builder(ctx, path, pred).aggregating_reader(SPECS, group_by=KEYS)
        answer = [(list(k), v) for k, v in r.aggregate()]
    elif arm == "aggregate_ungrouped":
        r = builder(ctx, path, pred).aggregating_reader(SPECS)
        answer = [([], r.aggregate())]
    else:
        r = builder(ctx, path, pred).build()
        t = pa.Table.from_batches(list(r))
        t = t.append_column("product", pc.multiply(t.column("l_extendedprice").cast(pa.decimal128(20, 2)), t.column("l_discount")))   # (decimal128(36, 4))
        g = t.group_by(KEYS).aggregate([([], "count_all"), ("l_quantity", "sum"), ("l_extendedprice", "sum"), ("l_discount", "sum"), ("product", "sum")])
        cols = [g.column(c).to_pylist() for c in KEYS + ["count_all", "l_quantity_sum", "l_extendedprice_sum", "l_discount_sum", "product_sum"]]
        answer = [(list(row[:2]), list(row[2:])) for row in zip(*cols)]
    dt = time.perf_counter() - t0
    d2h = r.d2h_bytes()
    r.close()
    return dt, sorted(answer, key=repr), d2h
ARMS = ["host_group_by", "aggregate_groups", "aggregate_ungrouped", "host_group_by_filter", "aggregate_groups_filter"]
if len(sys.argv) > 2 and sys.argv[1] == "--one-pass":  # the child under rocprofv3: one arm, one pass
    one_pass(capi.Context(0), sys.argv[3], sys.argv[2])
    sys.exit(0)
import pyarrow.orc as orc
import make_lineitem
from orc_rust_amd.gen import workloads as W
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 24_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "reader_group_by.json")
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "li.orc")
table = make_lineitem.arrow_table(W.lineitem_table(rows), rows)
orc.write_table(table, path, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
del table
ctx = capi.Context(0)
out = {"file": {"rows": rows, "bytes": os.path.getsize(path), "stripes": orc.ORCFile(path).nstripes, "writer": "ORC C++ (pyarrow.orc), zstd, 64 MiB stripes"},
       "projection": NAMES, "keys": KEYS, "specs": [repr(s) for s in SPECS], "filter": "l_quantity < 24", "batch_size": 65536, "prefetch": 2, "warmup": 1, "repeats": 3,
       "runs": []}
answers = {}
for arm in ARMS:
    one_pass(ctx, path, arm)
    passes = [one_pass(ctx, path, arm) for _ in range(3)]
    ms = [round(p[0] * 1e3, 1) for p in passes]
    answers[arm] = passes[0][1]
    assert all(p[1] == passes[0][1] for p in passes), arm       # the same answer on every pass
    out["runs"].append({"arm": arm, "groups": len(passes[0][1]), "answer": [[k, [str(x) for x in v]] for k, v in passes[0][1]], "d2h_bytes": passes[0][2],
                        "ms_best": min(ms), "ms_all": ms, "spread": round((max(ms) - min(ms)) / min(ms), 4)})
    print(out["runs"][-1], file=sys.stderr, flush=True)
by = {r["arm"]: r for r in out["runs"]}
same = lambda a, b: len(a) == len(b) and all(ka == kb and len(va) == len(vb) and all(D(x) == D(y) for x, y in zip(va, vb)) for (ka, va), (kb, vb) in zip(a, b))
assert same(answers["aggregate_groups"], answers["host_group_by"]), (answers["aggregate_groups"], answers["host_group_by"])
assert same(answers["aggregate_groups_filter"], answers["host_group_by_filter"]), (answers["aggregate_groups_filter"], answers["host_group_by_filter"])
assert by["aggregate_groups"]["d2h_bytes"] == 0 and by["aggregate_groups_filter"]["d2h_bytes"] == 0
ratio = lambda a, b: round(by[a]["ms_best"] / by[b]["ms_best"], 3)
out["ratios"] = {"aggregate_groups_vs_host_group_by": ratio("aggregate_groups", "host_group_by"), "aggregate_groups_vs_aggregate_ungrouped": ratio("aggregate_groups", "aggregate_ungrouped"),
                 "aggregate_groups_filter_vs_host_group_by_filter": ratio("aggregate_groups_filter", "host_group_by_filter")}
a, b = by["host_group_by"], by["aggregate_groups"]
out["groups_faster_than_host_by_more_than_its_spread"] = b["ms_best"] < a["ms_best"] / (1 + a["spread"])
if shutil.which("rocprofv3"):
    raw = os.path.join(tmp, "raw")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", raw, "--", sys.executable, os.path.abspath(__file__), "--one-pass",
                    "aggregate_groups", path], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    stats = list(csv.DictReader(open(glob.glob(os.path.join(raw, "**", "*kernel_stats.csv"), recursive=True)[0])))
    total = sum(float(r["TotalDurationNs"]) for r in stats)
    share = lambda word: round(sum(float(r["TotalDurationNs"]) for r in stats if word in r["Name"]) / total, 4)
    out["device_time_share"] = {"arm": "aggregate_groups", "group_assign_kernel": share("group_assign_kernel"), "group_number_kernel": share("group_number_kernel"),
                                "agg_group_partial_kernel": share("agg_group_partial_kernel"), "agg_group_final_kernel": share("agg_group_final_kernel"),
                                "all_kernels_ms": round(total / 1e6, 1)}
shutil.rmtree(tmp, ignore_errors=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
