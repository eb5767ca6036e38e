#!/usr/bin/env python3
"""What dictionary output buys: string columns handed out as dictionary<int32, string> (with_dictionary_columns / Arrow target 27)
against the plain Utf8 read, in one process.
  (a) the 24 M-row lineitem file of profiles/reader_device.py (ORC C++ writer, Zstandard, 64 MiB stripes,
      dictionary_key_size_threshold = 0.8) read whole through the host path:
        plain         every string column as Utf8 (twice: the two runs' difference is the run-to-run spread),
        dictionary    with_dictionary_columns on the string columns that EVERY stripe footer of the file says are DICTIONARY /
                      DICTIONARY_V2 there (read with tests/orcfile.py, no list in this script).
      Whole-file milliseconds and orcgpu_reader_d2h_bytes per arm.
  (b) the C3 stripe of gen/workloads.py (dictionary Utf8 + PRESENT, snappy) at 10 M rows through the C ABI's stage + decode, with the
      default target and with target 27: device milliseconds of the decode call (orcgpu_last_timing) and, of those, dict_emit_kernel's
      (orcgpu_last_lane_stats).
One warm-up pass per arm, then the best of three.
    python3 profiles/reader_dictionary.py [file rows] [C3 rows]      writes profiles/reader_dictionary.json"""
import json, os, sys, tempfile, time
import torch  # (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden")); sys.path.insert(0, os.path.join(ROOT, "tests"))
if not os.path.isdir("/usr/share/zoneinfo"):
    import tzdata; os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
import pyarrow.orc as orc
import make_lineitem
import orcfile
from orc_rust_amd import capi
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.gen import workloads as W
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 24_000_000
c3_rows = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
torch.cuda.init()
table = make_lineitem.arrow_table(W.lineitem_table(rows), rows)
print("table of %d rows made" % rows, file=sys.stderr, flush=True)
path = os.path.join(tempfile.mkdtemp(), "li.orc")
orc.write_table(table, path, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
arrow_bytes = table.nbytes
del table
print("file written: %d bytes" % os.path.getsize(path), file=sys.stderr, flush=True)
# ---- the columns: strings that are dictionary-encoded in every stripe, by the stripe footers ----
f = orcfile.OrcFile(path)
strings = [(n, c) for n, c, t in f.root_columns() if t.kind in (7, 16, 17)]
enc = {n: sorted({s.encodings[c][0] for s in f.stripes}) for n, c in strings}
dict_sizes = {n: max(s.encodings[c][1] for s in f.stripes) for n, c in strings}
chosen = [n for n, _ in strings if set(enc[n]) <= {1, 3}]
n_stripes = len(f.stripes)
del f
ctx = capi.Context(0)
def file_pass(names):
    b = ArrowReaderBuilder.try_new(path, ctx).with_batch_size(65536).with_prefetch(2)
    if names: b = b.with_dictionary_columns(names)
    r = b.build(); n = 0
    for batch in r:
        n += batch.num_rows
        del batch
    return n, r
def timed(names):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    n, r = file_pass(names)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    d2h = r.d2h_bytes(); r.close()
    return dt * 1e3, n, d2h
out = {"file": {"rows": rows, "bytes": os.path.getsize(path), "arrow_bytes": arrow_bytes, "stripes": n_stripes,
                "string_column_encodings": enc, "dictionary_columns": chosen, "dictionary_sizes": {n: dict_sizes[n] for n in chosen}},
       "batch_size": 65536, "prefetch": 2, "warmup": 1, "repeats": 3, "runs": []}
for name, names in (("plain", None), ("dictionary", chosen), ("plain_again", None)):
    timed(names)
    res = [timed(names) for _ in range(3)]
    best = min(t for t, _, _ in res)
    out["runs"].append({"arm": name, "rows": res[0][1], "ms_best": round(best, 1), "ms_all": [round(t, 1) for t, _, _ in res], "d2h_bytes": res[0][2]})
    print(out["runs"][-1], file=sys.stderr, flush=True)
ms = {r["arm"]: r["ms_best"] for r in out["runs"]}
d2h = {r["arm"]: r["d2h_bytes"] for r in out["runs"]}
out["plain_spread_ms"] = round(abs(ms["plain"] - ms["plain_again"]), 1)
out["dictionary_vs_plain_ms"] = round(ms["dictionary"] / min(ms["plain"], ms["plain_again"]), 3)
out["dictionary_vs_plain_d2h"] = round(d2h["dictionary"] / d2h["plain"], 3)
out["dictionary_faster_beyond_spread"] = ms["dictionary"] + out["plain_spread_ms"] < min(ms["plain"], ms["plain_again"])
os.remove(path)
# ---- (b) C3 at the stripe level ----
n, cols, streams, _ = W.c3_stripe(c3_rows, 0, "snappy", want_expect=False)
def c3_arm(target):
    c = [dict(cols[0], arrow_target=target)]
    staged = ctx.stage(n, streams, c, compression="snappy")
    res = None
    runs = []
    for k in range(4):  # (one warm-up, the result's buffers decoded into again)
        res = ctx.decode([staged], [res] if res is not None else None)[0]
        assert res.status()[0] == 0, res.status()
        total = ctx.timing()[0]
        emit = sum(l["dict_emit_kernel_ms"] for l in ctx.lane_stats())
        if k: runs.append((total, emit))
    ab = res.arrow_bytes
    res.free(); staged.free()
    best = min(runs)
    return {"device_ms_best": round(best[0], 3), "device_ms_all": [round(t, 3) for t, _ in runs], "dict_emit_kernel_ms": round(best[1], 3), "arrow_bytes": ab}
c3 = {"rows": n, "compression": "snappy", "default": c3_arm(0), "dictionary": c3_arm(27), "default_again": c3_arm(0)}
base = min(c3["default"]["device_ms_best"], c3["default_again"]["device_ms_best"])
c3["default_spread_ms"] = round(abs(c3["default"]["device_ms_best"] - c3["default_again"]["device_ms_best"]), 3)
c3["dictionary_vs_default_ms"] = round(c3["dictionary"]["device_ms_best"] / base, 3)
c3["dictionary_vs_default_arrow_bytes"] = round(c3["dictionary"]["arrow_bytes"] / c3["default"]["arrow_bytes"], 3)
out["c3"] = c3
print(c3, file=sys.stderr, flush=True)
with open(os.path.join(ROOT, "profiles", "reader_dictionary.json"), "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out))
