#!/usr/bin/env python3
"""What an IN row filter costs and saves the file reader: the lineitem file of profiles/reader_filter.py (ORC C++ writer,
Zstandard, 64 MiB stripes) read whole in one process: unfiltered, under l_shipmode IN ('MAIL', 'SHIP') (TPC-H Q12), under
l_orderkey IN 16, 1000 and 65536 keys drawn from the file, and -- for the lists of 2 and 16 values -- under the OR of the EQ
leaves, the only way to say the same without the IN leaf.  One warm-up pass per arm, then the best of three; d2h_bytes is what
the reader copied back, rows_kept what it handed out.  filter_in_kernel's share of the device time comes from a pass of the
65536-key arm in a child process of its own under rocprofv3 --kernel-trace --stats (left out where rocprofv3 is not there).
    python3 profiles/reader_filter_in.py [rows] [out.json]      writes profiles/reader_filter_in.json"""
import csv, glob, json, os, shutil, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
if not os.path.isdir("/usr/share/zoneinfo"):
    import tzdata; os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
import numpy as np
from orc_rust_amd import capi
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
def arms(keys):
    """keys: the file's distinct order keys, shuffled"""
    modes = [V.Utf8("MAIL"), V.Utf8("SHIP")]
    lists = {n: [V.Int64(int(k)) for k in keys[:n]] for n in (16, 1000, 65536)}
    return [("unfiltered", None), ("shipmode_in_2", P.in_list("l_shipmode", modes)), ("shipmode_or_2", P.or_([P.eq("l_shipmode", v) for v in modes])),
            ("orderkey_in_16", P.in_list("l_orderkey", lists[16])), ("orderkey_or_16", P.or_([P.eq("l_orderkey", v) for v in lists[16]])),
            ("orderkey_in_1000", P.in_list("l_orderkey", lists[1000])), ("orderkey_in_65536", P.in_list("l_orderkey", lists[65536]))]
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
    d2h = r.d2h_bytes()
    r.close()
    return dt, n, d2h
if len(sys.argv) > 2 and sys.argv[1] == "--one-pass":  # the child under rocprofv3: one arm, one pass
    one_pass(capi.Context(0), sys.argv[3], dict(arms(np.load(sys.argv[4])))[sys.argv[2]])
    sys.exit(0)
import pyarrow.orc as orc
import make_lineitem
from orc_rust_amd.gen import workloads as W
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 24_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "reader_filter_in.json")
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "li.orc")
table = make_lineitem.arrow_table(W.lineitem_table(rows), rows)
orc.write_table(table, path, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
keys = np.unique(table.column("l_orderkey").to_numpy())
np.random.default_rng(5).shuffle(keys)
keys = keys[:65536]
np.save(os.path.join(tmp, "keys.npy"), keys)
del table
ctx = capi.Context(0)
out = {"file": {"rows": rows, "bytes": os.path.getsize(path), "writer": "ORC C++ (pyarrow.orc), zstd, 64 MiB stripes"},
       "batch_size": 65536, "prefetch": 2, "warmup": 1, "repeats": 3, "runs": []}
for name, pred in arms(keys):
    one_pass(ctx, path, pred)
    passes = [one_pass(ctx, path, pred) for _ in range(3)]
    out["runs"].append({"arm": name, "rows_kept": passes[0][1], "d2h_bytes": passes[0][2], "ms_best": round(min(p[0] for p in passes) * 1e3, 1),
                        "ms_all": [round(p[0] * 1e3, 1) for p in passes]})
    print(out["runs"][-1], file=sys.stderr, flush=True)
by = {r["arm"]: r for r in out["runs"]}
base = by["unfiltered"]
out["unfiltered_spread"] = round((max(base["ms_all"]) - min(base["ms_all"])) / min(base["ms_all"]), 4)  # run to run, of the best
out["vs_unfiltered"] = {r["arm"]: {"time": round(r["ms_best"] / base["ms_best"], 3), "d2h_bytes": round(r["d2h_bytes"] / base["d2h_bytes"], 4)} for r in out["runs"][1:]}
out["in_vs_or_of_eq"] = {"shipmode_2": round(by["shipmode_in_2"]["ms_best"] / by["shipmode_or_2"]["ms_best"], 3),
                         "orderkey_16": round(by["orderkey_in_16"]["ms_best"] / by["orderkey_or_16"]["ms_best"], 3)}
assert by["shipmode_in_2"]["rows_kept"] == by["shipmode_or_2"]["rows_kept"] and by["orderkey_in_16"]["rows_kept"] == by["orderkey_or_16"]["rows_kept"]
if shutil.which("rocprofv3"):
    raw = os.path.join(tmp, "raw")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", raw, "--", sys.executable, os.path.abspath(__file__), "--one-pass",
                    "orderkey_in_65536", path, os.path.join(tmp, "keys.npy")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    stats = list(csv.DictReader(open(glob.glob(os.path.join(raw, "**", "*kernel_stats.csv"), recursive=True)[0])))
    total = sum(float(r["TotalDurationNs"]) for r in stats)
    share = lambda word: round(sum(float(r["TotalDurationNs"]) for r in stats if word in r["Name"]) / total, 4)
    out["device_time_share"] = {"arm": "orderkey_in_65536", "filter_in_kernel": share("filter_in_kernel"), "filter_eval_kernel": share("filter_eval_kernel"),
                                "filter_gather_kernel": share("filter_gather_kernel"), "all_kernels_ms": round(total / 1e6, 1)}
shutil.rmtree(tmp, ignore_errors=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
