#!/usr/bin/env python3
"""What TPC-H Q6 costs the file reader, five ways, in one process: the lineitem file of profiles/reader_filter.py (ORC C++ writer,
Zstandard, 64 MiB stripes), every arm on the projection l_quantity, l_extendedprice, l_discount (Decimal(15, 2)):
  (a) host_read            the unfiltered host read
  (b) filter_then_compute  the Q6-shaped row filter, then sum(l_extendedprice * l_discount) with pyarrow.compute on the kept rows
  (c) device_torch         device output, the product summed with torch on the low words of the Decimal128 values
  (d) aggregate_filter     aggregate([sum_product]) under the same filter
  (e) aggregate_all        aggregate([sum_product]) with no filter
One warm-up pass per arm, then the best of three with each arm's spread; per arm the bytes copied back and the host waits per
stripe (the filter's and the aggregation's one wait each: what the code does, not a measurement).  The kernels' shares of the
device time come from a pass of (d) in a child process of its own under rocprofv3 --kernel-trace --stats (left out where rocprofv3
is not there).
    python3 profiles/reader_aggregate.py [rows] [out.json]      writes profiles/reader_aggregate.json"""
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
NAMES = ["l_quantity", "l_extendedprice", "l_discount"]
Q6 = P.and_([P.gte("l_discount", V.Decimal128(D("0.05"))), P.lte("l_discount", V.Decimal128(D("0.07"))), P.lt("l_quantity", V.Decimal128(D("24")))])
SPEC = [Agg.sum_product("l_extendedprice", "l_discount"), Agg.count_rows()]
def builder(ctx, path, pred):
    b = ArrowReaderBuilder.try_new(path, ctx).with_batch_size(65536).with_prefetch(2).with_projection(NAMES)
    return b.with_row_filter(pred, prune=False) if pred is not None else b
def one_pass(ctx, path, arm):
    """(seconds, the arm's answer, bytes copied back)"""
    import pyarrow as pa, pyarrow.compute as pc
    t0 = time.perf_counter()
    if arm in ("aggregate_filter", "aggregate_all"):
        r = builder(ctx, path, Q6 if arm == "aggregate_filter" else None).aggregating_reader(SPEC)
        answer = r.aggregate()[0]
    elif arm == "device_torch":
        r = builder(ctx, path, None).with_device_output().build()
        acc = torch.zeros((), dtype=torch.int64, device="cuda")
        for batch in r:   # (Decimal(15, 2) fits the low word; a product of two fits int64 at these sizes: what a torch consumer would do)
            p, d = (batch.column(c).values[:, 0] for c in ("l_extendedprice", "l_discount"))   # (Decimal128: int64 [n, 2], low word first)
            acc += (p * d).sum()
        answer = D(int(acc.item())).scaleb(-4)
    else:
        r = builder(ctx, path, Q6 if arm == "filter_then_compute" else None).build()
        answer, n = D(0), 0
        for batch in r:
            n += batch.num_rows
            if arm == "filter_then_compute" and batch.num_rows:
                prod = pc.multiply(batch.column("l_extendedprice").cast(pa.decimal128(20, 2)), batch.column("l_discount"))   # (decimal128(36, 4))
                answer += pc.sum(prod).as_py() or D(0)
        if arm == "host_read":
            answer = n
    dt = time.perf_counter() - t0
    d2h = r.d2h_bytes()
    r.close()
    return dt, answer, d2h
ARMS = ["host_read", "filter_then_compute", "device_torch", "aggregate_filter", "aggregate_all"]
WAITS = {"host_read": 0, "filter_then_compute": 1, "device_torch": 0, "aggregate_filter": 1, "aggregate_all": 1}   # beyond the decode's own
if len(sys.argv) > 2 and sys.argv[1] == "--one-pass":  # the child under rocprofv3: one arm, one pass
    one_pass(capi.Context(0), sys.argv[3], sys.argv[2])
    sys.exit(0)
import pyarrow.orc as orc
import make_lineitem
from orc_rust_amd.gen import workloads as W
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 24_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "reader_aggregate.json")
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "li.orc")
table = make_lineitem.arrow_table(W.lineitem_table(rows), rows)
orc.write_table(table, path, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
del table
ctx = capi.Context(0)
out = {"file": {"rows": rows, "bytes": os.path.getsize(path), "stripes": orc.ORCFile(path).nstripes, "writer": "ORC C++ (pyarrow.orc), zstd, 64 MiB stripes"},
       "projection": NAMES, "columns": "Decimal(15, 2)", "batch_size": 65536, "prefetch": 2, "warmup": 1, "repeats": 3, "runs": []}
for arm in ARMS:
    one_pass(ctx, path, arm)
    passes = [one_pass(ctx, path, arm) for _ in range(3)]
    ms = [round(p[0] * 1e3, 1) for p in passes]
    out["runs"].append({"arm": arm, "answer": str(passes[0][1]), "d2h_bytes": passes[0][2], "filter_or_aggregate_waits_per_stripe": WAITS[arm], "ms_best": min(ms),
                        "ms_all": ms, "spread": round((max(ms) - min(ms)) / min(ms), 4)})
    print(out["runs"][-1], file=sys.stderr, flush=True)
by = {r["arm"]: r for r in out["runs"]}
assert by["aggregate_filter"]["answer"] == by["filter_then_compute"]["answer"], (by["aggregate_filter"]["answer"], by["filter_then_compute"]["answer"])
assert by["aggregate_all"]["answer"] == by["device_torch"]["answer"], (by["aggregate_all"]["answer"], by["device_torch"]["answer"])
assert by["aggregate_filter"]["d2h_bytes"] == 0 and by["aggregate_all"]["d2h_bytes"] == 0
ratio = lambda a, b: round(by[a]["ms_best"] / by[b]["ms_best"], 3)
out["ratios"] = {"aggregate_filter_vs_filter_then_compute": ratio("aggregate_filter", "filter_then_compute"), "aggregate_filter_vs_host_read": ratio("aggregate_filter", "host_read"),
                 "aggregate_all_vs_host_read": ratio("aggregate_all", "host_read"), "aggregate_all_vs_device_torch": ratio("aggregate_all", "device_torch"),
                 "filter_then_compute_vs_host_read": ratio("filter_then_compute", "host_read")}
if shutil.which("rocprofv3"):
    raw = os.path.join(tmp, "raw")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", raw, "--", sys.executable, os.path.abspath(__file__), "--one-pass",
                    "aggregate_filter", path], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    stats = list(csv.DictReader(open(glob.glob(os.path.join(raw, "**", "*kernel_stats.csv"), recursive=True)[0])))
    total = sum(float(r["TotalDurationNs"]) for r in stats)
    share = lambda word: round(sum(float(r["TotalDurationNs"]) for r in stats if word in r["Name"]) / total, 4)
    out["device_time_share"] = {"arm": "aggregate_filter", "agg_partial_kernel": share("agg_partial_kernel"), "agg_final_kernel": share("agg_final_kernel"),
                                "filter_eval_kernel": share("filter_eval_kernel"), "all_kernels_ms": round(total / 1e6, 1)}
shutil.rmtree(tmp, ignore_errors=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
