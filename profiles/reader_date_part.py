#!/usr/bin/env python3
"""What a date part in an expression (year(l_shipdate): AX_DATE_PART in device/agg_expr_eval.h) costs the file
reader, against the routes a caller had without it.

The lineitem file of profiles/reader_filter.py (ORC C++ writer, Zstandard, 64 MiB stripes; l_shipdate is a Date).  One process, a
warm-up and best of three per arm, every pass listed with the spread.  Each arm is held to the host route's answer BEFORE anything
is timed: a wrong arm ends the script.
  (a) Q7 / Q9-shaped: SUM(l_extendedprice * (1 - l_discount)) GROUP BY year(l_shipdate) -- `gpu`: l_year a computed column,
      Agg.sum(expr) grouped by it, nothing copied back; `host`: the two operands and the date read back, pyarrow.compute.year, the
      product and Table.group_by on the same box.  Both must give the same years and the same exact sums.
  (b) the row filter year(l_shipdate).eq(1995) -- `date_part`: the expression leaf (filter_expr_kernel, no pruning through year());
      `literal_dates`: l_shipdate >= 1995-01-01 AND l_shipdate < 1996-01-01, the two literal comparisons that keep the same rows,
      without pruning too, so that the leaf alone differs.  Both must keep the rows numpy keeps of the table the file was written
      from: the same count and the same sum of l_orderkey.
No mark is set in advance.
    python3 profiles/reader_date_part.py [rows] [out.json]      writes profiles/reader_date_part.json"""
import datetime, decimal, json, os, shutil, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
if not os.path.isdir("/usr/share/zoneinfo"):
    import tzdata; os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.orc as orc
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg, col, year
from orc_rust_amd.arrow_reader import ArrowReaderBuilder, concat_batches
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
REVENUE = col("l_extendedprice") * (1 - col("l_discount"))
GROUP_COLS = ["l_shipdate", "l_extendedprice", "l_discount"]
FILTER_COLS = ["l_orderkey", "l_shipdate"]
YEAR = 1995
EPOCH = datetime.date(1970, 1, 1).toordinal()
Y0, Y1 = datetime.date(YEAR, 1, 1).toordinal() - EPOCH, datetime.date(YEAR + 1, 1, 1).toordinal() - EPOCH
def builder(ctx, path, cols):
    return ArrowReaderBuilder.try_new(path, ctx).with_batch_size(65536).with_prefetch(2).with_projection(cols)
def group_gpu(ctx, path):
    t0 = time.perf_counter()
    groups = builder(ctx, path, GROUP_COLS).with_computed_columns({"l_year": year("l_shipdate")}).aggregate([Agg.sum(REVENUE)], group_by=["l_year"])
    return time.perf_counter() - t0, sorted((k[0], decimal.Decimal(v[0])) for k, v in groups)
def group_host(ctx, path):
    t0 = time.perf_counter()
    t = concat_batches(list(builder(ctx, path, GROUP_COLS).build()))
    rev = pc.multiply(t.column("l_extendedprice"), pc.subtract(pa.scalar(decimal.Decimal(1)), t.column("l_discount")))
    g = pa.table({"l_year": pc.year(t.column("l_shipdate")), "revenue": rev}).group_by("l_year").aggregate([("revenue", "sum")])
    return time.perf_counter() - t0, sorted(zip(g.column("l_year").to_pylist(), (decimal.Decimal(v) for v in g.column("revenue_sum").to_pylist())))
def filtered(ctx, path, pred):
    r = builder(ctx, path, FILTER_COLS).with_row_filter(pred, prune=False).build()
    t0 = time.perf_counter()
    n, keys = 0, 0
    for batch in r:
        n += batch.num_rows
        keys += int(pc.sum(batch.column("l_orderkey")).as_py() or 0)
    dt = time.perf_counter() - t0
    over = r.filter_overflow_rows()
    r.close()
    return dt, n, keys, over
import make_lineitem
from orc_rust_amd.gen import workloads as W
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 24_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "reader_date_part.json")
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "li.orc")
table = make_lineitem.arrow_table(W.lineitem_table(rows), rows)
orc.write_table(table, path, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
ship = table.column("l_shipdate").cast(pa.int32()).to_numpy()
in_year = (ship >= Y0) & (ship < Y1)
host_kept = int(in_year.sum())
host_keys = int(table.column("l_orderkey").to_numpy()[in_year].astype(object).sum()) if host_kept else 0
ctx = capi.Context(0)
out = {"file": {"rows": rows, "bytes": os.path.getsize(path)}, "batch_size": 65536, "prefetch": 2, "warmup": 1, "repeats": 3}
def timed(fn, *args):
    fn(*args)
    passes = [fn(*args) for _ in range(3)]
    ms = [p[0] * 1e3 for p in passes]
    return {"ms_best": round(min(ms), 1), "ms_all": [round(m, 1) for m in ms], "spread": round((max(ms) - min(ms)) / min(ms), 4)}
# (a): the gate, then the timing
want = group_host(ctx, path)[1]
got = group_gpu(ctx, path)[1]
assert got == want, "group by year(l_shipdate): the computed column and the host route give different years or sums:\n%r\n%r" % (got[:3], want[:3])
tg, th = timed(group_gpu, ctx, path), timed(group_host, ctx, path)
out["group_by_year"] = {"groups": len(want), "values_agree": True, "gpu": tg, "host": th, "gpu_over_host": round(tg["ms_best"] / th["ms_best"], 3)}
print(json.dumps(out["group_by_year"]))
# (b)
arms = [("date_part", year("l_shipdate").eq(YEAR)), ("literal_dates", P.and_([P.gte("l_shipdate", V.Int32(Y0)), P.lt("l_shipdate", V.Int32(Y1))]))]
for name, pred in arms:
    _, n, keys, over = filtered(ctx, path, pred)
    assert (n, keys, over) == (host_kept, host_keys, 0), "row filter %s: kept %d rows (key sum %d, %d overflows), numpy keeps %d (key sum %d)" % (name, n, keys, over, host_kept, host_keys)
res = {name: timed(filtered, ctx, path, pred) for name, pred in arms}
out["filter_year"] = {"year": YEAR, "rows_kept": host_kept, "rows_agree": True, **res,
                      "date_part_over_literal_dates": round(res["date_part"]["ms_best"] / res["literal_dates"]["ms_best"], 3)}
print(json.dumps(out["filter_year"]))
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
shutil.rmtree(tmp, ignore_errors=True)
