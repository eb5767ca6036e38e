#!/usr/bin/env python3
"""What FILTER (WHERE ...) per aggregate saves the file reader, and what it costs the aggregates that have none, in one process: the
lineitem file of profiles/reader_q1.py (ORC C++ writer, Zstandard, 64 MiB stripes).
(a) A Q14-shaped list on the projection l_shipinstruct (plain Utf8 reads), l_extendedprice, l_discount (Decimal(15, 2)) --
    lineitem has no p_type: l_shipinstruct LIKE 'DELIVER%' stands where Q14 has p_type LIKE 'PROMO%':
      one_drain   aggregate([sum(price * (1 - disc)) FILTER (WHERE l_shipinstruct LIKE 'DELIVER%'), sum(price * (1 - disc))])
      two_drains  what gives the same two numbers without conditions: aggregate([sum(price * (1 - disc))]) under the row filter
                  l_shipinstruct LIKE 'DELIVER%', then the same list without a filter -- two decodes of the file
    One warm-up pass per arm, then the best of three with each arm's spread.  Both arms must return the same two Decimals and copy
    no byte back: asserted.  agg_cond_eval_kernel's share of the device time comes from a pass of one_drain in a child process of
    its own under rocprofv3 --kernel-trace --stats, a run with no counters alongside (left out where rocprofv3 is not there).
(b) With --parent TREE LIB (a checkout of the parent commit and its built liborcgpu.so) the existing aggregates are timed on both
    builds, alternately, each turn a child process of its own with a warm-up and three passes: profiles/reader_aggregate.py's arms
    (d) aggregate_filter and (e) aggregate_all, profiles/reader_group_by.py's arm (b) aggregate_groups and profiles/reader_q1.py's
    arm (b) aggregate_q1.  The margin is the parent's own spread over its turns.
    python3 profiles/reader_aggregate_filter.py [rows] [out.json] [--parent TREE LIB]      writes profiles/reader_aggregate_filter.json"""
import csv, glob, json, os, shutil, subprocess, sys, tempfile, time
from decimal import Decimal as D
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB_CHILD = len(sys.argv) > 1 and sys.argv[1] == "--ab-child"      # --ab-child ROOT arm file: the tree to import is ROOT
ROOT = sys.argv[2] if AB_CHILD else HERE
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(HERE, "tests", "golden"))
if not os.path.isdir("/usr/share/zoneinfo"):
    import tzdata; os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
import torch
from orc_rust_amd import capi
from orc_rust_amd.aggregate import Agg, col
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
KEYS = ["l_returnflag", "l_linestatus"]
Q1_NAMES = KEYS + ["l_quantity", "l_extendedprice", "l_discount", "l_tax"]
NAMES = ["l_shipinstruct", "l_extendedprice", "l_discount"]
PRICE, DISC, TAX = col("l_extendedprice"), col("l_discount"), col("l_tax")
REVENUE = Agg.sum(PRICE * (1 - DISC))
PROMO = P.like("l_shipinstruct", "DELIVER%")
PLAIN = [Agg.count_rows(), Agg.sum("l_quantity"), Agg.sum("l_extendedprice"), Agg.sum("l_discount"), Agg.sum_product("l_extendedprice", "l_discount")]
Q1 = [Agg.sum("l_quantity"), Agg.sum("l_extendedprice"), Agg.sum(PRICE * (1 - DISC)), Agg.sum(PRICE * (1 - DISC) * (1 + TAX)), Agg.avg("l_quantity"),
      Agg.avg("l_extendedprice"), Agg.avg("l_discount"), Agg.count_rows()]
Q6 = P.and_([P.gte("l_discount", V.Decimal128(D("0.05"))), P.lte("l_discount", V.Decimal128(D("0.07"))), P.lt("l_quantity", V.Decimal128(D("24")))])
def builder(ctx, path, names, pred=None):
    b = ArrowReaderBuilder.try_new(path, ctx).with_batch_size(65536).with_prefetch(2).with_projection(names)
    return b.with_row_filter(pred, prune=False) if pred is not None else b
def ab_pass(ctx, path, arm):
    """one pass of an arm of the existing profiles, with their projections and specs"""
    t0 = time.perf_counter()
    if arm == "aggregate_q1":
        r = builder(ctx, path, Q1_NAMES).aggregating_reader(Q1, group_by=KEYS)
    elif arm == "aggregate_groups":
        r = builder(ctx, path, Q1_NAMES[:5]).aggregating_reader(PLAIN, group_by=KEYS)
    else:
        r = builder(ctx, path, Q1_NAMES[2:5], Q6 if arm == "aggregate_filter" else None).aggregating_reader([PLAIN[4], PLAIN[0]])
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
def drain(ctx, path, specs, pred=None):
    r = builder(ctx, path, NAMES, pred).aggregating_reader(specs)
    values, d2h = r.aggregate(), r.d2h_bytes()
    r.close()
    return values, d2h
def one_pass(ctx, path, arm):
    """(seconds, [the conditioned sum, the unconditioned sum], bytes copied back)"""
    t0 = time.perf_counter()
    if arm == "one_drain":
        answer, d2h = drain(ctx, path, [REVENUE.where(PROMO), REVENUE])
    else:
        (promo,), d1 = drain(ctx, path, [REVENUE], PROMO)
        (whole,), d2 = drain(ctx, path, [REVENUE])
        answer, d2h = [promo, whole], d1 + d2
    return time.perf_counter() - t0, answer, d2h
ARMS = ["one_drain", "two_drains"]
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
out_path = args[1] if len(args) > 1 else os.path.join(HERE, "profiles", "reader_aggregate_filter.json")
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "li.orc")
table = make_lineitem.arrow_table(W.lineitem_table(rows), rows)
orc.write_table(table, path, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
del table
out = {"file": {"rows": rows, "bytes": os.path.getsize(path), "stripes": orc.ORCFile(path).nstripes, "writer": "ORC C++ (pyarrow.orc), zstd, 64 MiB stripes"},
       "projection": NAMES, "specs": [repr(REVENUE.where(PROMO)), repr(REVENUE)], "batch_size": 65536, "prefetch": 2, "warmup": 1, "repeats": 3, "runs": []}
if parent:      # before this process opens the GPU: the existing aggregates on the parent's build and on this one, turn by turn
    ab = {}
    for turn in range(2):
        for arm in ("aggregate_filter", "aggregate_all", "aggregate_groups", "aggregate_q1"):
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
    out["runs"].append({"arm": arm, "answer": [str(x) for x in passes[0][1]], "d2h_bytes": passes[0][2], "ms_best": min(ms), "ms_all": ms,
                        "spread": round((max(ms) - min(ms)) / min(ms), 4)})
    print(out["runs"][-1], file=sys.stderr, flush=True)
by = {r["arm"]: r for r in out["runs"]}
assert answers["one_drain"] == answers["two_drains"] and all(isinstance(x, D) for x in answers["one_drain"]) and 0 < answers["one_drain"][0] < answers["one_drain"][1]
assert by["one_drain"]["d2h_bytes"] == 0 and by["two_drains"]["d2h_bytes"] == 0
out["ratios"] = {"one_drain_vs_two_drains": round(by["one_drain"]["ms_best"] / by["two_drains"]["ms_best"], 3)}
if shutil.which("rocprofv3"):
    raw = os.path.join(tmp, "raw")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", raw, "--", sys.executable, os.path.abspath(__file__), "--one-pass",
                    "one_drain", path], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    stats = list(csv.DictReader(open(glob.glob(os.path.join(raw, "**", "*kernel_stats.csv"), recursive=True)[0])))
    total = sum(float(r["TotalDurationNs"]) for r in stats)
    share = lambda word: round(sum(float(r["TotalDurationNs"]) for r in stats if r["Name"].startswith(word)) / total, 4)
    out["device_time_share"] = {"arm": "one_drain", "agg_cond_eval_kernel": share("agg_cond_eval_kernel"), "filter_like_kernel": share("filter_like_kernel"),
                                "agg_partial_kernel": share("agg_partial_kernel"), "agg_expr_partial_kernel": share("agg_expr_partial_kernel"),
                                "agg_final_kernel": share("agg_final_kernel"), "all_kernels_ms": round(total / 1e6, 1)}
shutil.rmtree(tmp, ignore_errors=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
