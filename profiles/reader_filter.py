#!/usr/bin/env python3
"""What the row filter buys the file reader: the 24 M-row lineitem file of profiles/reader_rate.py (ORC C++ writer, Zstandard,
64 MiB stripes) read whole three ways -- unfiltered, under a keep-all filter, and under filters on l_partkey that keep about
10 % and about 1 % of the rows, spread over every row group (statistics cannot prune there) --, with prune=False and with
prune=True.  Every exported batch is released at once (no Arrow import inside the timed passes).  One warm-up pass (it pins the
host buffers), then the best and the median of five.  "arrow_bytes" is what the batches handed out hold -- what was copied
back, bar alignment --, counted in a pass of its own.
    python3 profiles/reader_filter.py [rows]      writes profiles/reader_filter.json"""
import ctypes as C, json, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
if not os.path.isdir("/usr/share/zoneinfo"):
    import tzdata; os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
import numpy as np
import pyarrow as pa
import pyarrow.orc as orc
import make_lineitem
from orc_rust_amd import capi
from orc_rust_amd.gen import workloads as W
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 24_000_000
table = make_lineitem.arrow_table(W.lineitem_table(rows), rows)
path = os.path.join(tempfile.mkdtemp(), "li.orc")
orc.write_table(table, path, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
partkey = table.column("l_partkey").to_numpy()
cut10, cut1 = int(np.quantile(partkey, 0.10)), int(np.quantile(partkey, 0.01))
arrow_bytes = table.nbytes
del table, partkey
ctx = capi.Context(0)
L = ctx.L
class ArrowArray(C.Structure):
    _fields_ = [("length", C.c_int64), ("null_count", C.c_int64), ("offset", C.c_int64), ("n_buffers", C.c_int64), ("n_children", C.c_int64),
                ("buffers", C.c_void_p), ("children", C.c_void_p), ("dictionary", C.c_void_p), ("release", C.CFUNCTYPE(None, C.c_void_p)), ("private_data", C.c_void_p)]
class ArrowSchema(C.Structure):
    _fields_ = [("format", C.c_char_p), ("name", C.c_char_p), ("metadata", C.c_void_p), ("flags", C.c_int64), ("n_children", C.c_int64),
                ("children", C.c_void_p), ("dictionary", C.c_void_p), ("release", C.CFUNCTYPE(None, C.c_void_p)), ("private_data", C.c_void_p)]
ARMS = [("unfiltered", None), ("keep_all", P.gte("l_partkey", V.Int64(0))), ("keep_10pct", P.lte("l_partkey", V.Int64(cut10))),
        ("keep_1pct", P.lte("l_partkey", V.Int64(cut1)))]
def one_pass(pred, prune, count_bytes=False):
    h = C.c_void_p()
    assert L.orcgpu_reader_open_file(ctx.h, path.encode(), C.byref(h)) == 0
    L.orcgpu_reader_set_batch_size(h, 65536); L.orcgpu_reader_set_prefetch(h, 2)
    if pred is not None:
        nodes, keep = pred.flatten()
        assert L.orcgpu_reader_set_row_filter(h, nodes, len(nodes)) == 0
        if prune: assert L.orcgpu_reader_set_predicate(h, nodes, len(nodes)) == 0
    t0 = time.perf_counter(); n = nb = nbytes = 0
    while True:
        a, s = ArrowArray(), ArrowSchema()
        rc = L.orcgpu_reader_next_batch(h, C.byref(a), C.byref(s))
        if rc == 110: break  # ORCGPU_END_OF_FILE
        assert rc == 0, (rc, ctx.error())
        n += a.length; nb += 1
        if count_bytes:
            nbytes += pa.RecordBatch._import_from_c(C.addressof(a), C.addressof(s)).get_total_buffer_size()
        else:
            a.release(C.addressof(a)); s.release(C.addressof(s))
    dt = time.perf_counter() - t0
    L.orcgpu_reader_close(h)
    return dt, n, nb, nbytes
out = {"file": {"rows": rows, "bytes": os.path.getsize(path), "arrow_bytes": arrow_bytes}, "batch_size": 65536, "prefetch": 2, "warmup": 1, "repeats": 5, "runs": []}
for name, pred in ARMS:
    for prune in ((False,) if pred is None else (False, True)):
        one_pass(pred, prune)
        ts = []
        for _ in range(5):
            dt, n, nb, _ = one_pass(pred, prune)
            ts.append(dt * 1e3)
        nbytes = one_pass(pred, prune, count_bytes=True)[3]
        out["runs"].append({"arm": name, "prune": prune, "rows_kept": n, "batches": nb, "arrow_bytes": nbytes, "ms_best": round(min(ts), 1),
                            "ms_median": round(statistics.median(ts), 1)})
        print(out["runs"][-1], file=sys.stderr, flush=True)
base = next(r for r in out["runs"] if r["arm"] == "unfiltered")["ms_median"]
out["vs_unfiltered"] = {"%s%s" % (r["arm"], "_prune" if r["prune"] else ""): round(r["ms_median"] / base, 3) for r in out["runs"] if r["arm"] != "unfiltered"}
with open(os.path.join(ROOT, "profiles", "reader_filter.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
