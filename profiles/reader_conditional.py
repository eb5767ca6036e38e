#!/usr/bin/env python3
"""What the conditionals of an expression (when / case / coalesce / nullif / abs: AX_CMP .. AX_PUSH_NULL in
device/agg_expr_eval.h) cost the file reader, against the routes a caller had without them.

The lineitem file of profiles/reader_filter.py (ORC C++ writer, Zstandard, 64 MiB stripes).  One process an arm (this script starts
itself once per arm), a warm-up and best of three, every pass listed with the spread.  Each arm is held to the host route's answer
BEFORE anything is timed: a wrong arm ends the script.
  (a) COUNT(*), SUM(l_extendedprice) GROUP BY CASE WHEN l_quantity < 10 THEN 0 WHEN l_quantity < 25 THEN 1 ELSE 2 END -- `gpu`: the
      bucket a computed column (compute_columns_cond_kernel), grouped by on the device; `host`: the two columns read back,
      pyarrow.compute.case_when, Table.group_by on the same box.
  (b) SUM(l_extendedprice / NULLIF(l_quantity - 1, 0)) -- `gpu`: Agg.sum of the expression (agg_expr_cond_partial_kernel), a
      Decimal at scale 6 rounded half away from zero, nothing copied back; `host`: the two columns read back, the divisor's zeros
      made NULL with pyarrow.compute.if_else, pyarrow.compute.divide (sixteen digits, truncated), rounded to six digits half away
      from zero, pyarrow.compute.sum.
No mark is set in advance.
    python3 profiles/reader_conditional.py [rows] [out.json]      writes profiles/reader_conditional.json"""
import decimal, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
if not os.path.isdir("/usr/share/zoneinfo"):
    import tzdata; os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.orc as orc
COLS = ["l_quantity", "l_extendedprice"]
def builder(ctx, path):
    from orc_rust_amd.arrow_reader import ArrowReaderBuilder
    return ArrowReaderBuilder.try_new(path, ctx).with_batch_size(65536).with_prefetch(2).with_projection(COLS)
def bucket_gpu(ctx, path):
    from orc_rust_amd.aggregate import Agg, case, col
    t0 = time.perf_counter()
    q = col("l_quantity")
    groups = builder(ctx, path).with_computed_columns({"bucket": case([(q < 10, 0), (q < 25, 1)], 2)}).aggregate([Agg.count_rows(), Agg.sum("l_extendedprice")], group_by=["bucket"])
    return time.perf_counter() - t0, sorted((k[0], v[0], str(decimal.Decimal(v[1]).normalize())) for k, v in groups)
def bucket_host(ctx, path):
    from orc_rust_amd.arrow_reader import concat_batches
    t0 = time.perf_counter()
    t = concat_batches(list(builder(ctx, path).build()))
    q = t.column("l_quantity")
    ten, twenty_five = (pa.scalar(decimal.Decimal(v), q.type) for v in (10, 25))
    b = pc.case_when(pc.make_struct(pc.less(q, ten), pc.less(q, twenty_five)), pa.scalar(0, pa.int64()), pa.scalar(1, pa.int64()), pa.scalar(2, pa.int64()))
    g = pa.table({"b": b, "p": t.column("l_extendedprice")}).group_by("b").aggregate([("p", "count"), ("p", "sum")])
    return time.perf_counter() - t0, sorted(zip(g.column("b").to_pylist(), g.column("p_count").to_pylist(), (str(decimal.Decimal(v).normalize()) for v in g.column("p_sum").to_pylist())))
def guarded_gpu(ctx, path):
    from orc_rust_amd.aggregate import Agg, col, nullif
    t0 = time.perf_counter()
    total, = builder(ctx, path).aggregate([Agg.sum(col("l_extendedprice") / nullif(col("l_quantity") - 1, 0))])
    return time.perf_counter() - t0, [str(decimal.Decimal(total).normalize())]
def guarded_host(ctx, path):
    from orc_rust_amd.arrow_reader import concat_batches
    t0 = time.perf_counter()
    t = concat_batches(list(builder(ctx, path).build()))
    d = pc.subtract(t.column("l_quantity"), pa.scalar(decimal.Decimal(1), t.column("l_quantity").type))
    d = pc.if_else(pc.equal(d, pa.scalar(decimal.Decimal(0), d.type)), pa.scalar(None, d.type), d)
    total = pc.sum(pc.round(pc.divide(t.column("l_extendedprice"), d), 6, round_mode="half_towards_infinity")).as_py()
    return time.perf_counter() - t0, [str(decimal.Decimal(total).normalize())]
ARMS = {"case_bucket.gpu": bucket_gpu, "case_bucket.host": bucket_host, "guarded_division.gpu": guarded_gpu, "guarded_division.host": guarded_host}
def run_arm(name, path):
    """in a process of its own: the gate against the host route, a warm-up, three passes -> one JSON line"""
    from orc_rust_amd import capi
    ctx = capi.Context(0)
    fn, host = ARMS[name], ARMS[name.split(".")[0] + ".host"]
    want = host(ctx, path)[1]
    got = fn(ctx, path)[1]
    assert got == want, "%s: the arm and the host route differ:\n%r\n%r" % (name, got[:3], want[:3])
    fn(ctx, path)
    ms = [fn(ctx, path)[0] * 1e3 for _ in range(3)]
    print(json.dumps({"groups": len(want), "values_agree": True, "ms_best": round(min(ms), 1), "ms_all": [round(m, 1) for m in ms], "spread": round((max(ms) - min(ms)) / min(ms), 4)}))
if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--arm":
        run_arm(sys.argv[2], sys.argv[3])
        sys.exit(0)
    import make_lineitem
    from orc_rust_amd.gen import workloads as W
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 24_000_000
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "reader_conditional.json")
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "li.orc")
    orc.write_table(make_lineitem.arrow_table(W.lineitem_table(rows), rows), path, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
    out = {"file": {"rows": rows, "bytes": os.path.getsize(path)}, "batch_size": 65536, "prefetch": 2, "warmup": 1, "repeats": 3, "one_process_an_arm": True}
    try:
        for name in ARMS:
            line = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", name, path], check=True, capture_output=True, text=True, timeout=900).stdout.strip().splitlines()[-1]
            out.setdefault(name.split(".")[0], {})[name.split(".")[1]] = json.loads(line)
            print(name, line, flush=True)
        for k in ("case_bucket", "guarded_division"):
            out[k]["gpu_over_host"] = round(out[k]["gpu"]["ms_best"] / out[k]["host"]["ms_best"], 3)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
