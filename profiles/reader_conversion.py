#!/usr/bin/env python3
"""What the conversions of an expression (cast / round_ / floor / ceil / trunc: AX_TO_F64 .. AX_F64_ROUND in
device/agg_expr_eval.h's mixed interpreter) cost the file reader, against the routes a caller had without them.

The lineitem file of profiles/reader_filter.py (ORC C++ writer, Zstandard, 64 MiB stripes).  One process an arm (this script starts
itself once per arm), a warm-up and best of three, every pass listed with the spread.  Each arm is held to the host route's answer
BEFORE anything is timed: a wrong arm ends the script.
  (a) SUM(CAST(l_quantity AS DOUBLE) * CAST(l_discount AS DOUBLE)) -- `gpu`: Agg.sum of the expression
      (agg_expr_conv_partial_kernel), nothing copied back; `host`: the two columns read back, pyarrow.compute.cast to float64,
      multiply, sum.  Both Decimals are exact doubles' neighbours and the sum's order differs: the two are compared to 1e-9 relative.
  (b) COUNT(*), SUM(l_extendedprice) GROUP BY CAST(FLOOR(l_extendedprice / 1000) AS BIGINT) -- `gpu`: the bucket a computed column
      (compute_columns_conv_kernel), grouped by on the device; `host`: the column read back, divided, floored and cast with
      pyarrow.compute, Table.group_by on the same box.
No mark is set in advance.
With `--parent TREE` (a built checkout of the parent commit) the three existing expression profiles -- reader_q1.py,
reader_filter_expr.py, reader_conditional.py -- are re-run too, in the same session: each at the parent (its own script, its own
library) and then at this tree, same row count; every timed arm of theirs (every record with an `ms_best`) goes to
`existing_profiles` as {parent, new, new_over_parent} with both spreads beside the ratio, and
`no_slower_than_parent_within_its_spread` says what the spread allows to conclude.
    python3 profiles/reader_conversion.py [rows] [out.json] [--parent TREE]      writes profiles/reader_conversion.json"""
import decimal, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
if not os.path.isdir("/usr/share/zoneinfo"):
    import tzdata; os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.orc as orc
COLS = ["l_quantity", "l_discount", "l_extendedprice"]
def builder(ctx, path):
    from orc_rust_amd.arrow_reader import ArrowReaderBuilder
    return ArrowReaderBuilder.try_new(path, ctx).with_batch_size(65536).with_prefetch(2).with_projection(COLS)
def product_gpu(ctx, path):
    from orc_rust_amd.aggregate import Agg, cast
    t0 = time.perf_counter()
    total, = builder(ctx, path).aggregate([Agg.sum(cast("l_quantity", "float64") * cast("l_discount", "float64"))])
    return time.perf_counter() - t0, [total]
def product_host(ctx, path):
    from orc_rust_amd.arrow_reader import concat_batches
    t0 = time.perf_counter()
    t = concat_batches(list(builder(ctx, path).build()))
    total = pc.sum(pc.multiply(pc.cast(t.column("l_quantity"), pa.float64()), pc.cast(t.column("l_discount"), pa.float64()))).as_py()
    return time.perf_counter() - t0, [total]
def bucket_gpu(ctx, path):
    from orc_rust_amd.aggregate import Agg, cast, col, floor
    t0 = time.perf_counter()
    groups = builder(ctx, path).with_computed_columns({"bucket": cast(floor(col("l_extendedprice") / 1000), "int64")}).aggregate(
        [Agg.count_rows(), Agg.sum("l_extendedprice")], group_by=["bucket"])
    return time.perf_counter() - t0, sorted((k[0], v[0], str(decimal.Decimal(v[1]).normalize())) for k, v in groups)
def bucket_host(ctx, path):
    from orc_rust_amd.arrow_reader import concat_batches
    t0 = time.perf_counter()
    p = concat_batches(list(builder(ctx, path).build())).column("l_extendedprice")
    b = pc.cast(pc.floor(pc.divide(p, pa.scalar(decimal.Decimal(1000), pa.decimal128(4, 0)))), pa.int64())
    g = pa.table({"b": b, "p": p}).group_by("b").aggregate([("p", "count"), ("p", "sum")])
    return time.perf_counter() - t0, sorted(zip(g.column("b").to_pylist(), g.column("p_count").to_pylist(), (str(decimal.Decimal(v).normalize()) for v in g.column("p_sum").to_pylist())))
ARMS = {"double_product.gpu": product_gpu, "double_product.host": product_host, "floor_bucket.gpu": bucket_gpu, "floor_bucket.host": bucket_host}
def agree(got, want):
    if len(got) == 1 and isinstance(got[0], float):
        return abs(got[0] - want[0]) <= 1e-9 * abs(want[0])
    return got == want
def run_arm(name, path):
    """in a process of its own: the gate against the host route, a warm-up, three passes -> one JSON line"""
    from orc_rust_amd import capi
    ctx = capi.Context(0)
    fn, host = ARMS[name], ARMS[name.split(".")[0] + ".host"]
    want = host(ctx, path)[1]
    got = fn(ctx, path)[1]
    assert agree(got, want), "%s: the arm and the host route differ:\n%r\n%r" % (name, got[:3], want[:3])
    fn(ctx, path)
    ms = [fn(ctx, path)[0] * 1e3 for _ in range(3)]
    print(json.dumps({"groups": len(want), "values_agree": True, "ms_best": round(min(ms), 1), "ms_all": [round(m, 1) for m in ms], "spread": round((max(ms) - min(ms)) / min(ms), 4)}))
EXISTING = ("reader_q1", "reader_filter_expr", "reader_conditional")
def timed(node, at=""):
    """every record of a profile's JSON that holds an `ms_best`, by its path"""
    out = {}
    if isinstance(node, dict):
        if "ms_best" in node:
            out[(at + ":" + str(node["arm"])) if "arm" in node else at] = {"ms_best": node["ms_best"], "spread": node.get("spread")}
        for k, v in node.items():
            out.update(timed(v, at + "/" + str(k)))
    elif isinstance(node, list):
        for k, v in enumerate(node):
            out.update(timed(v, "%s[%d]" % (at, k)))
    return out
def existing_profiles(parent, rows, tmp):
    """the three profiles at the parent's tree and at this one -> {profile: {arm: {parent, new, new_over_parent, ...}}}"""
    res = {}
    for name in EXISTING:
        got = {}
        for build, tree in (("parent", parent), ("new", ROOT)):
            out = os.path.join(tmp, "%s.%s.json" % (name, build))
            env = dict(os.environ)
            env.pop("ORCGPU_LIB", None)
            subprocess.run([sys.executable, os.path.join(tree, "profiles", name + ".py"), str(rows), out], check=True, cwd=tree, env=env, stdout=subprocess.DEVNULL, timeout=3000)
            with open(out) as f:
                got[build] = timed(json.load(f))
        res[name] = {}
        for arm in sorted(set(got["parent"]) & set(got["new"])):
            a, b = got["parent"][arm], got["new"][arm]
            res[name][arm] = {"parent": a, "new": b, "new_over_parent": round(b["ms_best"] / a["ms_best"], 4),
                              "no_slower_than_parent_within_its_spread": b["ms_best"] <= a["ms_best"] * (1 + (a["spread"] or 0.0))}
        print(name, json.dumps(res[name]), flush=True)
    return res
if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--arm":
        run_arm(sys.argv[2], sys.argv[3])
        sys.exit(0)
    parent = None
    if "--parent" in sys.argv:
        k = sys.argv.index("--parent")
        parent = os.path.abspath(sys.argv[k + 1])
        del sys.argv[k:k + 2]
    import make_lineitem
    from orc_rust_amd.gen import workloads as W
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 24_000_000
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "reader_conversion.json")
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "li.orc")
    orc.write_table(make_lineitem.arrow_table(W.lineitem_table(rows), rows), path, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
    out = {"file": {"rows": rows, "bytes": os.path.getsize(path)}, "batch_size": 65536, "prefetch": 2, "warmup": 1, "repeats": 3, "one_process_an_arm": True}
    try:
        for name in ARMS:
            line = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", name, path], check=True, capture_output=True, text=True, timeout=900).stdout.strip().splitlines()[-1]
            out.setdefault(name.split(".")[0], {})[name.split(".")[1]] = json.loads(line)
            print(name, line, flush=True)
        for k in ("double_product", "floor_bucket"):
            out[k]["gpu_over_host"] = round(out[k]["gpu"]["ms_best"] / out[k]["host"]["ms_best"], 3)
        if parent:
            out["existing_profiles"] = existing_profiles(parent, rows, tmp)
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
