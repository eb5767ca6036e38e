#!/usr/bin/env python3
"""What an expression leaf of the row filter (Predicate.compare: lhs OP rhs) costs the file reader: the lineitem file of
profiles/reader_filter.py (ORC C++ writer, Zstandard, 64 MiB stripes; its date columns are Date, its money columns Decimal(15, 2))
read whole in one process under four arms:
  (a) unfiltered
  (b) two literal comparisons on Date columns, l_shipdate < X AND l_commitdate > 0, X chosen so that about as many rows are kept
      as under (c): the yardstick -- what (c) and (d) are measured against is this arm of the same run
  (c) TPC-H Q12's two column-against-column leaves, l_commitdate < l_receiptdate AND l_shipdate < l_commitdate
  (d) l_extendedprice * (1 - l_discount) > X, X the 90th percentile of the product: about 10 % kept
One warm-up pass per arm, then the best of three with every pass listed.  rows_kept is what the reader handed out, rows_host what
numpy keeps of the same columns of the table the file was written from; they must agree.  filter_expr_kernel's share of the device
time comes from a pass of arm (c) in a child process of its own under rocprofv3 --kernel-trace --stats (left out where rocprofv3 is
not there).
    python3 profiles/reader_filter_expr.py [rows] [out.json]      writes profiles/reader_filter_expr.json"""
import csv, decimal, glob, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
if not os.path.isdir("/usr/share/zoneinfo"):
    import tzdata; os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
from orc_rust_amd import capi
from orc_rust_amd.aggregate import col, lit
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
def arms(ship_before, revenue_above):
    """ship_before: days; revenue_above: the unscaled threshold at scale 4"""
    return [("unfiltered", None),
            ("literal_dates", P.and_([P.lt("l_shipdate", V.Int32(ship_before)), P.gt("l_commitdate", V.Int32(0))])),
            ("q12_column_vs_column", P.and_([col("l_commitdate") < col("l_receiptdate"), col("l_shipdate") < col("l_commitdate")])),
            ("revenue_above", col("l_extendedprice") * (1 - col("l_discount")) > lit(decimal.Decimal(revenue_above).scaleb(-4)))]
def one_pass(ctx, path, pred):
    b = ArrowReaderBuilder.try_new(path, ctx).with_batch_size(65536).with_prefetch(2)
    if pred is not None:
        b = b.with_row_filter(pred, prune=False)
    r = b.build()
    t0 = time.perf_counter()
    n = 0
    for batch in r:
        n += batch.num_rows
    dt = time.perf_counter() - t0
    d2h, over = r.d2h_bytes(), r.filter_overflow_rows()
    r.close()
    return dt, n, d2h, over
if len(sys.argv) > 2 and sys.argv[1] == "--one-pass":  # the child under rocprofv3: one arm, one pass
    one_pass(capi.Context(0), sys.argv[3], dict(arms(int(sys.argv[4]), int(sys.argv[5])))[sys.argv[2]])
    sys.exit(0)
import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import make_lineitem
from orc_rust_amd.gen import workloads as W
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 24_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "reader_filter_expr.json")
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "li.orc")
table = make_lineitem.arrow_table(W.lineitem_table(rows), rows)
orc.write_table(table, path, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
# the host's answers, from the table the file was written from: dates as days, money as unscaled int64 (Decimal(15, 2) fits)
days = {c: table.column(c).cast(pa.int32()).to_numpy() for c in ("l_shipdate", "l_commitdate", "l_receiptdate")}
def unscaled(c):
    return np.frombuffer(table.column(c).combine_chunks().buffers()[1], dtype=np.int64)[::2][:rows].copy()
price, disc = unscaled("l_extendedprice"), unscaled("l_discount")
types = {c: str(table.schema.field(c).type) for c in ("l_shipdate", "l_commitdate", "l_receiptdate", "l_extendedprice", "l_discount")}
del table
q12 = (days["l_commitdate"] < days["l_receiptdate"]) & (days["l_shipdate"] < days["l_commitdate"])
ship_before = int(np.quantile(days["l_shipdate"], q12.mean()))
revenue = price * (100 - disc)  # scale 2 + 2
revenue_above = int(np.quantile(revenue, 0.9))
host = {"unfiltered": rows, "literal_dates": int(((days["l_shipdate"] < ship_before) & (days["l_commitdate"] > 0)).sum()), "q12_column_vs_column": int(q12.sum()),
        "revenue_above": int((revenue > revenue_above).sum())}
ARMS = arms(ship_before, revenue_above)
ctx = capi.Context(0)
out = {"file": {"rows": rows, "bytes": os.path.getsize(path), "writer": "ORC C++ (pyarrow.orc), zstd, 64 MiB stripes", "types": types},
       "literals": {"ship_before_days": ship_before, "revenue_above_unscaled_scale_4": revenue_above},
       "batch_size": 65536, "prefetch": 2, "warmup": 1, "repeats": 3, "runs": []}
for name, pred in ARMS:
    one_pass(ctx, path, pred)
    passes = [one_pass(ctx, path, pred) for _ in range(3)]
    ms = [p[0] * 1e3 for p in passes]
    out["runs"].append({"arm": name, "rows_kept": passes[0][1], "rows_host": host[name], "rows_agree": passes[0][1] == host[name], "overflow_rows": passes[0][3],
                        "d2h_bytes": passes[0][2], "ms_best": round(min(ms), 1), "ms_all": [round(m, 1) for m in ms], "spread": round((max(ms) - min(ms)) / min(ms), 4)})
    print(out["runs"][-1], file=sys.stderr, flush=True)
yard = out["runs"][1]
out["vs_literal_dates"] = {r["arm"]: round(r["ms_best"] / yard["ms_best"], 3) for r in out["runs"][2:]}
if shutil.which("rocprofv3"):
    raw = os.path.join(tmp, "raw")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", raw, "--", sys.executable, os.path.abspath(__file__), "--one-pass",
                    "q12_column_vs_column", path, str(ship_before), str(revenue_above)], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    stats = list(csv.DictReader(open(glob.glob(os.path.join(raw, "**", "*kernel_stats.csv"), recursive=True)[0])))
    total = sum(float(r["TotalDurationNs"]) for r in stats)
    share = lambda word: round(sum(float(r["TotalDurationNs"]) for r in stats if word in r["Name"]) / total, 4)
    out["device_time_share"] = {"arm": "q12_column_vs_column", "filter_expr_kernel": share("filter_expr_kernel"), "filter_eval_kernel": share("filter_eval_kernel"),
                                "filter_gather_kernel": share("filter_gather_kernel"), "all_kernels_ms": round(total / 1e6, 1)}
shutil.rmtree(tmp, ignore_errors=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
