#!/usr/bin/env python3
"""What device-resident batches buy a consumer on the same GPU: the 24 M-row lineitem file of profiles/reader_filter.py (ORC C++
writer, Zstandard, 64 MiB stripes) read whole, in one process,
  host          the host path: every batch exported from pinned host memory and released at once (twice: the two runs' difference
                is the run-to-run spread the other arms are read against),
  device_sum    with_device_output(), every batch consumed on the device: values.sum() of every numeric column,
  device_write  with_device_output(), every batch handed to ArrowWriter.write_device into a sink that only counts bytes (the
                writer on a context of its own; without the three Date32 columns, which the writer does not take).
One warm-up pass per arm, then the best of three.  d2h_bytes: orcgpu_reader_d2h_bytes at the end of a pass.
    python3 profiles/reader_device.py [rows]      writes profiles/reader_device.json"""
import json, os, sys, tempfile, time
import torch  # (before liborcgpu.so is loaded: torch finds the GPU only when its HIP runtime is the process's first)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
if not os.path.isdir("/usr/share/zoneinfo"):
    import tzdata; os.environ["TZDIR"] = os.path.join(os.path.dirname(tzdata.__file__), "zoneinfo")
import pyarrow as pa
import pyarrow.orc as orc
import make_lineitem
from orc_rust_amd import capi
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.arrow_writer import ArrowWriterBuilder
from orc_rust_amd.gen import workloads as W
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 24_000_000
torch.cuda.init()
table = make_lineitem.arrow_table(W.lineitem_table(rows), rows)
path = os.path.join(tempfile.mkdtemp(), "li.orc")
orc.write_table(table, path, compression="zstd", dictionary_key_size_threshold=0.8, stripe_size=64 << 20)
arrow_bytes = table.nbytes
no_dates = [f.name for f in table.schema if not pa.types.is_date(f.type)]
del table
ctx, wctx = capi.Context(0), capi.Context(0)
class CountingSink:
    def __init__(self): self.n = 0
    def write(self, b): self.n += len(b)
def reader(device, names=None):
    b = ArrowReaderBuilder.try_new(path, ctx).with_batch_size(65536).with_prefetch(2)
    if names is not None: b = b.with_projection(names)
    return (b.with_device_output() if device else b).build()
def host_pass():
    r = reader(False); n = 0
    for batch in r:
        n += batch.num_rows
        del batch
    return n, r
def device_sum_pass():
    r = reader(True); n = 0; acc = []
    for batch in r:
        n += batch.num_rows
        for i in range(batch.num_columns):
            v = batch.column(i).values
            if v is not None and v.dtype != torch.bool: acc.append(v.sum())
        batch.release()
    total = torch.stack([a.to(torch.float64) for a in acc]).sum().item()  # (the sums are observed: one wait for all of them)
    return n, r
def device_write_pass():
    r = reader(True, no_dates); n = 0; w = None; sink = CountingSink()
    for batch in r:
        n += batch.num_rows
        if w is None: w = ArrowWriterBuilder(sink, batch.schema, ctx=wctx).with_compression("snappy").try_build()
        w.write_device(batch)
        batch.release()
    w.close(); w.free()
    return n, r
def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    n, r = fn()
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    d2h = r.d2h_bytes(); r.close()
    return dt * 1e3, n, d2h
out = {"file": {"rows": rows, "bytes": os.path.getsize(path), "arrow_bytes": arrow_bytes}, "batch_size": 65536, "prefetch": 2, "warmup": 1, "repeats": 3, "runs": []}
for name, fn in (("host", host_pass), ("device_sum", device_sum_pass), ("device_write", device_write_pass), ("host_again", host_pass)):
    timed(fn)
    res = [timed(fn) for _ in range(3)]
    best = min(t for t, _, _ in res)
    out["runs"].append({"arm": name, "rows": res[0][1], "ms_best": round(best, 1), "ms_all": [round(t, 1) for t, _, _ in res], "d2h_bytes": res[0][2],
                        "arrow_gb_per_s": round(arrow_bytes / best / 1e6, 1) if name != "device_write" else None})
    print(out["runs"][-1], file=sys.stderr, flush=True)
ms = {r["arm"]: r["ms_best"] for r in out["runs"]}
out["host_spread_ms"] = round(abs(ms["host"] - ms["host_again"]), 1)
out["device_sum_vs_host"] = round(ms["device_sum"] / min(ms["host"], ms["host_again"]), 3)
out["device_not_slower_than_host"] = ms["device_sum"] <= max(ms["host"], ms["host_again"]) + out["host_spread_ms"]
with open(os.path.join(ROOT, "profiles", "reader_device.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
