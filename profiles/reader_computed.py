#!/usr/bin/env python3
"""What a computed column costs the file reader, against evaluating the same expression in its consumer.

The lineitem file of profiles/reader_filter.py (ORC C++ writer, Zstandard, 64 MiB stripes).  revenue = l_extendedprice * (1 -
l_discount), a Decimal128(38, 4) computed column (16 bytes a row, materialised once per stripe by compute_columns_kernel; a decode
call with computed columns runs on ONE column lane, which is part of what is measured).  One process, a warm-up and best of three
per arm, every pass listed with the spread:
  (a) Q1-shaped: GROUP BY l_returnflag, l_linestatus under l_shipdate <= 1998-09-02 with SUM(l_quantity), SUM(l_extendedprice),
      SUM(revenue), COUNT(*) -- `computed`: revenue a computed column and Agg.sum('revenue'); `in_consumer`: Agg.sum(expr), the
      expression evaluated per kept row inside the reduction.  Both must give the same groups and values.
  (b) ORDER BY revenue DESC, l_orderkey, l_linenumber LIMIT 100 -- `top_k` on the computed column against the full read of the
      operands with the product and pyarrow.compute.select_k_unstable on the host.  Both arms must return the same rows.
  (c) device output with the computed column against device output of the operands plus the same product in torch ON DOUBLES:
      a different computation (inexact, 8 bytes a row), reported as such, not as the same work.
  (d) the share of compute_columns_kernel of the device time, from a pass of (a) `computed` in a child process of its own under
      rocprofv3 --kernel-trace --stats (left out where rocprofv3 is not there).
No mark is set in advance: (a) may well come out slower than Agg.sum(expr).
    python3 profiles/reader_computed.py [rows] [out.json]      writes profiles/reader_computed.json"""
import csv, decimal, glob, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
if not os.path.isdir("/usr/share/zoneinfo"):
    import tzdata; os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.orc as orc
import torch
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg, col
from orc_rust_amd.arrow_reader import ArrowReaderBuilder, concat_batches
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
from orc_rust_amd.top_k import SortKey
REVENUE = col("l_extendedprice") * (1 - col("l_discount"))
SHIP_BEFORE = 10471  # 1998-09-02 as days since 1970-01-01
Q1_COLS = ["l_returnflag", "l_linestatus", "l_quantity", "l_extendedprice", "l_discount", "l_shipdate"]
TOP_COLS = ["l_orderkey", "l_linenumber", "l_extendedprice", "l_discount"]
K = 100
def builder(ctx, path, cols):
    return ArrowReaderBuilder.try_new(path, ctx).with_batch_size(65536).with_prefetch(2).with_projection(cols)
def q1(ctx, path, computed):
    t0 = time.perf_counter()
    b = builder(ctx, path, Q1_COLS).with_row_filter(P.lte("l_shipdate", V.Int32(SHIP_BEFORE)), prune=False)
    specs = [Agg.sum("l_quantity"), Agg.sum("l_extendedprice"), Agg.sum("revenue") if computed else Agg.sum(REVENUE), Agg.count_rows()]
    if computed:
        b = b.with_computed_columns({"revenue": REVENUE})
    groups = b.aggregate(specs, group_by=["l_returnflag", "l_linestatus"])
    return time.perf_counter() - t0, sorted((k, tuple(v)) for k, v in groups)
def top_gpu(ctx, path):
    t0 = time.perf_counter()
    t = builder(ctx, path, TOP_COLS).with_computed_columns({"revenue": REVENUE}).top_k([SortKey("revenue", descending=True), SortKey("l_orderkey"), SortKey("l_linenumber")], K)
    return time.perf_counter() - t0, list(zip(t.column("l_orderkey").to_pylist(), t.column("l_linenumber").to_pylist(), t.column("revenue").to_pylist()))
def top_host(ctx, path):
    t0 = time.perf_counter()
    t = concat_batches(list(builder(ctx, path, TOP_COLS).build()))
    rev = pc.multiply(t.column("l_extendedprice"), pc.subtract(pa.scalar(decimal.Decimal(1)), t.column("l_discount")))
    t = t.append_column("revenue", rev)
    top = pc.select_k_unstable(t, K, [("revenue", "descending"), ("l_orderkey", "ascending"), ("l_linenumber", "ascending")])
    t = t.take(top)
    return time.perf_counter() - t0, list(zip(t.column("l_orderkey").to_pylist(), t.column("l_linenumber").to_pylist(), t.column("revenue").to_pylist()))
def low_words(c):
    v = c.values  # Decimal128: int64 [n, 2], low word first; these values fit the low word
    return v[:, 0]
def device(ctx, path, computed):
    t0 = time.perf_counter()
    b = builder(ctx, path, ["l_extendedprice", "l_discount"]).with_device_output()
    if computed:
        b = b.with_computed_columns({"revenue": REVENUE})
    total, rows = 0.0, 0
    for batch in b.build():
        if computed:
            r = low_words(batch.column("revenue")).double() / 1e4
        else:  # the same product, on doubles, in the consumer
            r = (low_words(batch.column("l_extendedprice")).double() / 100.0) * (1.0 - low_words(batch.column("l_discount")).double() / 100.0)
        total += float(r.sum())
        rows += batch.num_rows
    torch.cuda.synchronize()
    return time.perf_counter() - t0, rows, total
if len(sys.argv) > 2 and sys.argv[1] == "--one-pass":  # the child under rocprofv3: (a) computed, one pass
    q1(capi.Context(0), sys.argv[2], True)
    sys.exit(0)
import make_lineitem
from orc_rust_amd.gen import workloads as W
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 24_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "reader_computed.json")
tmp = tempfile.mkdtemp()
lineitem = os.path.join(tmp, "li.orc")
orc.write_table(make_lineitem.arrow_table(W.lineitem_table(rows), rows), lineitem, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
ctx = capi.Context(0)
out = {"file": {"rows": rows, "bytes": os.path.getsize(lineitem)}, "batch_size": 65536, "prefetch": 2, "warmup": 1, "repeats": 3}
def timed(fn, *args):
    fn(*args)
    passes = [fn(*args) for _ in range(3)]
    ms = [p[0] * 1e3 for p in passes]
    return passes[0], {"ms_best": round(min(ms), 1), "ms_all": [round(m, 1) for m in ms], "spread": round((max(ms) - min(ms)) / min(ms), 4)}
# (a)
pa_, ta = timed(q1, ctx, lineitem, True)
pb_, tb = timed(q1, ctx, lineitem, False)
assert pa_[1] == pb_[1], "Q1: the computed column and Agg.sum(expr) give different groups or values"
out["q1"] = {"groups": len(pa_[1]), "values_agree": True, "computed": ta, "in_consumer": tb, "computed_over_in_consumer": round(ta["ms_best"] / tb["ms_best"], 3)}
print(json.dumps(out["q1"]))
# (b)
pg, tg = timed(top_gpu, ctx, lineitem)
ph, th = timed(top_host, ctx, lineitem)
assert [(a, b, decimal.Decimal(c)) for a, b, c in pg[1]] == [(a, b, decimal.Decimal(c)) for a, b, c in ph[1]], "top-k: the two arms return different rows"
out["top_k"] = {"k": K, "rows_agree": True, "top_k": tg, "host": th, "top_k_over_host": round(tg["ms_best"] / th["ms_best"], 3)}
print(json.dumps(out["top_k"]))
# (c)
pc_, tc = timed(device, ctx, lineitem, True)
pd_, td = timed(device, ctx, lineitem, False)
assert pc_[1] == pd_[1] == rows
out["device_output"] = {"note": "a different computation: the exact Decimal128(38, 4) column against a product of doubles in torch", "computed": tc, "torch_doubles": td,
                        "sum_computed": pc_[2], "sum_torch_doubles": pd_[2], "computed_over_torch": round(tc["ms_best"] / td["ms_best"], 3)}
print(json.dumps(out["device_output"]))
# (d)
if shutil.which("rocprofv3"):
    prof = os.path.join(tmp, "prof")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "-o", "computed", "--", sys.executable, os.path.abspath(__file__), "--one-pass", lineitem],
                   check=False, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    total, mine = 0.0, 0.0
    for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            ns = float(row.get("TotalDurationNs", 0) or 0)
            total += ns
            if row.get("Name", "").startswith("compute_columns_kernel"):
                mine += ns
    if total:
        out["kernel_trace"] = {"arm": "q1 computed", "device_ms": round(total / 1e6, 1), "compute_columns_kernel_ms": round(mine / 1e6, 2), "compute_columns_kernel_share": round(mine / total, 5)}
json.dump(out, open(out_path, "w"), indent=1)
shutil.rmtree(tmp, ignore_errors=True)
