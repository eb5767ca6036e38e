#!/usr/bin/env python3
"""What ORDER BY ... LIMIT k on the GPU saves the file reader, in one process: the lineitem file of profiles/reader_q1.py (ORC C++
writer, Zstandard, 64 MiB stripes), ORDER BY l_extendedprice DESC LIMIT 100 on the projection l_orderkey, l_quantity,
l_extendedprice, l_discount, l_shipdate -- with no predicate, and under the Q6 predicate of profiles/reader_aggregate.py.
      top_k      builder.with_top_k(...): every stripe hands out its 100 best rows, top_k_order() merges them, one `take`
      host_sort  the only way to the same answer without it: the row filter (or the full read), every kept row copied back, then
                 pyarrow.compute.select_k_unstable on the host (the cheapest host way: a partial sort, not a full one)
One warm-up pass per arm, then the best of three with each arm's spread; wall time of the whole call and the reader's d2h_bytes().
Both arms must return the same 100 prices: asserted.
    python3 profiles/reader_top_k.py [rows] [out.json]      writes profiles/reader_top_k.json"""
import json, os, shutil, sys, tempfile, time
from decimal import Decimal as D
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(HERE, "tests", "golden"))
if not os.path.isdir("/usr/share/zoneinfo"):
    import tzdata; os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
import torch  # noqa: F401
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.orc as orc
from orc_rust_amd import capi
from orc_rust_amd.arrow_reader import ArrowReaderBuilder, concat_batches
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
from orc_rust_amd.top_k import SortKey
import make_lineitem
from orc_rust_amd.gen import workloads as W
NAMES = ["l_orderkey", "l_quantity", "l_extendedprice", "l_discount", "l_shipdate"]
Q6 = P.and_([P.gte("l_discount", V.Decimal128(D("0.05"))), P.lte("l_discount", V.Decimal128(D("0.07"))), P.lt("l_quantity", V.Decimal128(D("24")))])
K = 100
def builder(ctx, path, pred):
    b = ArrowReaderBuilder.try_new(path, ctx).with_batch_size(65536).with_prefetch(2).with_projection(NAMES)
    return b.with_row_filter(pred, prune=False) if pred is not None else b
def one_pass(ctx, path, arm, pred):
    """(seconds, the answer's prices, bytes copied back, rows copied back)"""
    t0 = time.perf_counter()
    if arm == "top_k":
        r = builder(ctx, path, pred).with_top_k([SortKey("l_extendedprice", descending=True)], K).build()
        table = concat_batches(list(r))
        rows = table.num_rows
        table = table.take(pa.array(r.top_k_order(), type=pa.uint64()))
    else:
        r = builder(ctx, path, pred).build()
        table = concat_batches(list(r))
        rows = table.num_rows
        table = table.take(pc.select_k_unstable(table, K, [("l_extendedprice", "descending")]))
    dt = time.perf_counter() - t0
    d2h = r.d2h_bytes()
    r.close()
    return dt, table.column("l_extendedprice").to_pylist(), d2h, rows
args = sys.argv[1:]
rows = int(args[0]) if args else 24_000_000
out_path = args[1] if len(args) > 1 else os.path.join(HERE, "profiles", "reader_top_k.json")
tmp = tempfile.mkdtemp()
path = os.path.join(tmp, "li.orc")
table = make_lineitem.arrow_table(W.lineitem_table(rows), rows)
orc.write_table(table, path, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
del table
out = {"file": {"rows": rows, "bytes": os.path.getsize(path), "stripes": orc.ORCFile(path).nstripes, "writer": "ORC C++ (pyarrow.orc), zstd, 64 MiB stripes"},
       "projection": NAMES, "order_by": "l_extendedprice DESC", "k": K, "batch_size": 65536, "prefetch": 2, "warmup": 1, "repeats": 3, "runs": []}
ctx = capi.Context(0)
for name, pred in (("no_predicate", None), ("q6", Q6)):
    answers = {}
    for arm in ("top_k", "host_sort"):
        one_pass(ctx, path, arm, pred)
        passes = [one_pass(ctx, path, arm, pred) for _ in range(3)]
        ms = [round(p[0] * 1e3, 1) for p in passes]
        assert all(p[1] == passes[0][1] for p in passes), (name, arm)       # the same answer on every pass
        answers[arm] = passes[0][1]
        out["runs"].append({"predicate": name, "arm": arm, "rows_copied_back": passes[0][3], "d2h_bytes": passes[0][2], "ms_best": min(ms), "ms_all": ms,
                            "spread": round((max(ms) - min(ms)) / min(ms), 4)})
        print(out["runs"][-1], file=sys.stderr, flush=True)
    assert answers["top_k"] == answers["host_sort"] and len(answers["top_k"]) == K, name
    a, b = out["runs"][-2], out["runs"][-1]
    assert a["d2h_bytes"] < b["d2h_bytes"], name
    out.setdefault("ratios", {})[name] = {"ms_top_k_over_host_sort": round(a["ms_best"] / b["ms_best"], 3), "d2h_top_k_over_host_sort": round(a["d2h_bytes"] / b["d2h_bytes"], 6)}
shutil.rmtree(tmp, ignore_errors=True)
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
