#!/usr/bin/env python3
"""TPC-H Q1's select list through the file reader, in one process: the lineitem file of profiles/reader_aggregate.py (ORC C++ writer,
Zstandard, 64 MiB stripes), every arm on the projection l_returnflag, l_linestatus (plain Utf8 reads), l_quantity, l_extendedprice,
l_discount, l_tax (Decimal(15, 2)), grouped by l_returnflag, l_linestatus:
  (a) host_q1          the host read, then pyarrow computing the two expression columns and Table.group_by(...).aggregate(...); the
                       averages from pyarrow's exact sums and counts, at scale + 4, half away from zero
  (b) aggregate_q1     aggregate() with Q1's eight aggregates: sum(l_quantity), sum(l_extendedprice), sum(price * (1 - disc)),
                       sum(price * (1 - disc) * (1 + tax)), avg(l_quantity), avg(l_extendedprice), avg(l_discount), count(*)
  (c) aggregate_plain  the five plain aggregates of profiles/reader_group_by.py by the same keys: the price of the expressions is (b) - (c)
One warm-up pass per arm, then the best of three with each arm's spread.  (a) and (b) must return the same groups, Decimals and
averages: asserted.  The kernels' shares of the device time come from a pass of (b) in a child process of its own under rocprofv3
--kernel-trace --stats, a run with no counters alongside (left out where rocprofv3 is not there).

With --parent TREE LIB (a checkout of the parent commit and its built liborcgpu.so) the existing aggregates are timed on both
builds, alternately, each turn a child process of its own with a warm-up and three passes: profiles/reader_aggregate.py's arms (d)
aggregate_filter and (e) aggregate_all, profiles/reader_group_by.py's arm (b) aggregate_groups.  The new build may not be slower than
the parent by more than the parent's own spread over its turns.
    python3 profiles/reader_q1.py [rows] [out.json] [--parent TREE LIB]      writes profiles/reader_q1.json"""
import csv, glob, json, os, shutil, subprocess, sys, tempfile, time
from decimal import Decimal as D, ROUND_HALF_UP
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB_CHILD = len(sys.argv) > 1 and sys.argv[1] == "--ab-child"      # --ab-child ROOT arm file: the tree to import is ROOT
ROOT = sys.argv[2] if AB_CHILD else HERE
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(HERE, "tests", "golden"))
if not os.path.isdir("/usr/share/zoneinfo"):
    import tzdata; os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
import torch
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
KEYS = ["l_returnflag", "l_linestatus"]
NAMES = KEYS + ["l_quantity", "l_extendedprice", "l_discount", "l_tax"]
PLAIN = [Agg.count_rows(), Agg.sum("l_quantity"), Agg.sum("l_extendedprice"), Agg.sum("l_discount"), Agg.sum_product("l_extendedprice", "l_discount")]
Q6 = P.and_([P.gte("l_discount", V.Decimal128(D("0.05"))), P.lte("l_discount", V.Decimal128(D("0.07"))), P.lt("l_quantity", V.Decimal128(D("24")))])
def builder(ctx, path, names, pred=None):
    b = ArrowReaderBuilder.try_new(path, ctx).with_batch_size(65536).with_prefetch(2).with_projection(names)
    return b.with_row_filter(pred, prune=False) if pred is not None else b
def ab_pass(ctx, path, arm):
    """one pass of an arm of the existing profiles, with their projections and specs"""
    t0 = time.perf_counter()
    if arm == "aggregate_groups":
        r = builder(ctx, path, NAMES[:5]).aggregating_reader(PLAIN, group_by=KEYS)
    else:
        r = builder(ctx, path, NAMES[2:5], Q6 if arm == "aggregate_filter" else None).aggregating_reader([PLAIN[4], PLAIN[0]])
    answer = r.aggregate()
    dt = time.perf_counter() - t0
    r.close()
    return dt, repr(answer)
if AB_CHILD:
    ctx = capi.Context(0)
    ab_pass(ctx, sys.argv[4], sys.argv[3])
    passes = [ab_pass(ctx, sys.argv[4], sys.argv[3]) for _ in range(3)]
    print(json.dumps({"ms": [round(p[0] * 1e3, 2) for p in passes], "answer": passes[0][1]}))
    sys.exit(0)
from orc_rust_amd.aggregate import col
PRICE, DISC, TAX = col("l_extendedprice"), col("l_discount"), col("l_tax")
Q1 = [Agg.sum("l_quantity"), Agg.sum("l_extendedprice"), Agg.sum(PRICE * (1 - DISC)), Agg.sum(PRICE * (1 - DISC) * (1 + TAX)), Agg.avg("l_quantity"),
      Agg.avg("l_extendedprice"), Agg.avg("l_discount"), Agg.count_rows()]
def one_pass(ctx, path, arm):
    """(seconds, the arm's answer as a sorted list of (keys, values), bytes copied back)"""
    import pyarrow as pa, pyarrow.compute as pc
    t0 = time.perf_counter()
    if arm == "aggregate_q1":
        r = builder(ctx, path, NAMES).aggregating_reader(Q1, group_by=KEYS)
        answer = [(list(k), v) for k, v in r.aggregate()]
    elif arm == "aggregate_plain":
        r = builder(ctx, path, NAMES).aggregating_reader(PLAIN, group_by=KEYS)
        answer = [(list(k), v) for k, v in r.aggregate()]
    else:
        r = builder(ctx, path, NAMES).build()
        t = pa.Table.from_batches(list(r))
        one = pa.scalar(D("1.00"), pa.decimal128(3, 2))
        disc_price = pc.multiply(t.column("l_extendedprice"), pc.subtract(one, t.column("l_discount"))).cast(pa.decimal128(24, 4))
        charge = pc.multiply(disc_price, pc.add(one, t.column("l_tax")).cast(pa.decimal128(5, 2)))     # (decimal128(30, 6))
        t = t.append_column("disc_price", disc_price).append_column("charge", charge)
        g = t.group_by(KEYS).aggregate([("l_quantity", "sum"), ("l_extendedprice", "sum"), ("disc_price", "sum"), ("charge", "sum"), ("l_discount", "sum"),
                                        ("l_quantity", "count"), ([], "count_all")])
        cols = [g.column(c).to_pylist() for c in KEYS + ["l_quantity_sum", "l_extendedprice_sum", "disc_price_sum", "charge_sum", "l_discount_sum", "l_quantity_count",
                                                         "count_all"]]
        avg = lambda total, n: (total / n).quantize(D(1).scaleb(-6), rounding=ROUND_HALF_UP)      # (exact division at precision 60, then half away from zero)
        answer = []
        import decimal
        with decimal.localcontext() as c:
            c.prec = 60
            for k1, k2, qty, price, dp, ch, disc, n, rows in zip(*cols):       # (no NULLs in lineitem: every count is the group's rows)
                answer.append(([k1, k2], [qty, price, dp, ch, avg(qty, n), avg(price, n), avg(disc, n), rows]))
    dt = time.perf_counter() - t0
    d2h = r.d2h_bytes()
    r.close()
    return dt, sorted(answer, key=repr), d2h
ARMS = ["host_q1", "aggregate_q1", "aggregate_plain"]
if len(sys.argv) > 2 and sys.argv[1] == "--one-pass":  # the child under rocprofv3: one arm, one pass
    one_pass(capi.Context(0), sys.argv[3], sys.argv[2])
    sys.exit(0)
import pyarrow.orc as orc
import make_lineitem
from orc_rust_amd.gen import workloads as W
args = sys.argv[1:]
parent = None
if "--parent" in args:
    k = args.index("--parent")
    parent = (os.path.abspath(args[k + 1]), os.path.abspath(args[k + 2]))
    del args[k:k + 3]
rows = int(args[0]) if args else 24_000_000
out_path = args[1] if len(args) > 1 else os.path.join(HERE, "profiles", "reader_q1.json")
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "li.orc")
table = make_lineitem.arrow_table(W.lineitem_table(rows), rows)
orc.write_table(table, path, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
del table
out = {"file": {"rows": rows, "bytes": os.path.getsize(path), "stripes": orc.ORCFile(path).nstripes, "writer": "ORC C++ (pyarrow.orc), zstd, 64 MiB stripes"},
       "projection": NAMES, "keys": KEYS, "q1_specs": [repr(s) for s in Q1], "plain_specs": [repr(s) for s in PLAIN], "batch_size": 65536, "prefetch": 2, "warmup": 1,
       "repeats": 3, "runs": []}
if parent:      # before this process opens the GPU: the existing aggregates on the parent's build and on this one, turn by turn
    ab = {}
    for turn in range(2):
        for arm in ("aggregate_filter", "aggregate_all", "aggregate_groups"):
            for build, (tree, lib) in (("parent", parent), ("new", (HERE, None))):
                env = dict(os.environ)
                env.pop("ORCGPU_LIB", None)
                if lib:
                    env["ORCGPU_LIB"] = lib
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", tree, arm, path], env=env, stdout=subprocess.PIPE, timeout=600, check=True)
                got = json.loads(p.stdout.decode().strip().splitlines()[-1])
                e = ab.setdefault(arm, {}).setdefault(build, {"ms_all": [], "answer": got["answer"]})
                assert e["answer"] == got["answer"], (arm, build)
                e["ms_all"] += got["ms"]
                print(arm, build, got["ms"], file=sys.stderr, flush=True)
    out["existing_aggregates_parent_against_new"] = {"method": "child processes, parent and new alternately, 2 turns of a warm-up and 3 passes each", "arms": {}}
    for arm, e in ab.items():
        assert e["parent"]["answer"] == e["new"]["answer"], arm      # the same values from both builds
        line = {}
        for build in ("parent", "new"):
            ms = e[build]["ms_all"]
            line[build] = {"ms_best": min(ms), "ms_all": ms, "spread": round((max(ms) - min(ms)) / min(ms), 4)}
        line["new_over_parent"] = round(line["new"]["ms_best"] / line["parent"]["ms_best"], 4)
        line["no_slower_than_parent_within_its_spread"] = line["new"]["ms_best"] <= line["parent"]["ms_best"] * (1 + line["parent"]["spread"])
        out["existing_aggregates_parent_against_new"]["arms"][arm] = line
ctx = capi.Context(0)
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
a, b = answers["host_q1"], answers["aggregate_q1"]
assert len(a) == len(b) and len(a) > 0
for (ka, va), (kb, vb) in zip(a, b):      # the same groups, Decimals and averages: values and scales
    assert ka == kb and len(va) == len(vb), (ka, kb)
    for x, y in zip(va, vb):
        assert D(x) == D(y) and (not isinstance(y, D) or D(x).as_tuple().exponent == y.as_tuple().exponent), (ka, x, y)
assert by["aggregate_q1"]["d2h_bytes"] == 0 and by["aggregate_plain"]["d2h_bytes"] == 0
ratio = lambda x, y: round(by[x]["ms_best"] / by[y]["ms_best"], 3)
out["ratios"] = {"aggregate_q1_vs_host_q1": ratio("aggregate_q1", "host_q1"), "aggregate_q1_vs_aggregate_plain": ratio("aggregate_q1", "aggregate_plain")}
if shutil.which("rocprofv3"):
    raw = os.path.join(tmp, "raw")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", raw, "--", sys.executable, os.path.abspath(__file__), "--one-pass",
                    "aggregate_q1", path], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    stats = list(csv.DictReader(open(glob.glob(os.path.join(raw, "**", "*kernel_stats.csv"), recursive=True)[0])))
    total = sum(float(r["TotalDurationNs"]) for r in stats)
    share = lambda word: round(sum(float(r["TotalDurationNs"]) for r in stats if r["Name"].startswith(word)) / total, 4)
    out["device_time_share"] = {"arm": "aggregate_q1", "group_assign_kernel": share("group_assign_kernel"), "group_number_kernel": share("group_number_kernel"),
                                "agg_group_partial_kernel": share("agg_group_partial_kernel"), "agg_group_expr_partial_kernel": share("agg_group_expr_partial_kernel"),
                                "agg_group_final_kernel": share("agg_group_final_kernel"), "all_kernels_ms": round(total / 1e6, 1)}
shutil.rmtree(tmp, ignore_errors=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
