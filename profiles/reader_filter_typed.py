#!/usr/bin/env python3
"""What a Decimal / Timestamp row filter costs and saves the file reader: a lineitem-shaped file -- l_orderkey Int64, l_quantity,
l_extendedprice, l_discount, l_tax Decimal128(12, 2), l_shipdate Timestamp -- written by this project's ArrowWriter, read whole
three ways in one process: unfiltered, under a keep-all Decimal filter (l_quantity >= 0.00), and under the filter of TPC-H Q6
(l_discount BETWEEN 0.05 AND 0.07 AND l_quantity < 24, one year of l_shipdate).  One warm-up pass per arm, then the best of
three; d2h_bytes is what the reader copied back, rows_kept what it handed out.
    python3 profiles/reader_filter_typed.py [rows] [out.json]      writes profiles/reader_filter_typed.json"""
import datetime, decimal, json, os, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import pyarrow as pa
from orc_rust_amd import capi
from orc_rust_amd.arrow_reader import ArrowReaderBuilder
from orc_rust_amd.arrow_writer import ArrowWriterBuilder
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V
D = decimal.Decimal
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 8_000_000
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "reader_filter_typed.json")
rng = np.random.default_rng(6)
DEC = pa.decimal128(12, 2)
def dec(unscaled):  # non-negative int64 unscaled values -> Decimal128(12, 2), without a Python object per row
    words = np.zeros((len(unscaled), 2), dtype="<i8")
    words[:, 0] = unscaled
    return pa.Array.from_buffers(DEC, len(unscaled), [None, pa.py_buffer(words.tobytes())])
schema = pa.schema([("l_orderkey", pa.int64()), ("l_quantity", DEC), ("l_extendedprice", DEC), ("l_discount", DEC), ("l_tax", DEC),
                    ("l_shipdate", pa.timestamp("ns"))])
day0 = int((datetime.datetime(1992, 1, 2) - datetime.datetime(1970, 1, 1)).total_seconds())
ctx = capi.Context(0)
path = os.path.join(tempfile.mkdtemp(), "lineitem_typed.orc")
with open(path, "wb") as f:
    w = ArrowWriterBuilder(f, schema, ctx=ctx).with_row_index_stride(10000).try_build()
    for at in range(0, rows, 1 << 20):
        n = min(1 << 20, rows - at)
        qty = rng.integers(1, 51, n)
        w.write(pa.RecordBatch.from_arrays([pa.array(np.arange(at, at + n, dtype=np.int64) // 4), dec(qty * 100), dec(qty * rng.integers(90000, 200001, n)),
                                            dec(rng.integers(0, 11, n)), dec(rng.integers(0, 9, n)),
                                            pa.array((day0 + rng.integers(0, 2526, n) * 86400) * 10 ** 9, pa.timestamp("ns"))], schema=schema))
    w.close()
    w.free()
year = lambda y: V.TimestampNs(datetime.datetime(y, 1, 1))
ARMS = [("unfiltered", None), ("keep_all_decimal", P.gte("l_quantity", V.Decimal128(D("0.00")))),
        ("q6", P.and_([P.gte("l_shipdate", year(1994)), P.lt("l_shipdate", year(1995)), P.gte("l_discount", V.Decimal128(D("0.05"))),
                       P.lte("l_discount", V.Decimal128(D("0.07"))), P.lt("l_quantity", V.Decimal128(D("24")))]))]
def one_pass(pred):
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
out = {"file": {"rows": rows, "bytes": os.path.getsize(path), "writer": "ArrowWriter, uncompressed, row index stride 10000"}, "batch_size": 65536, "prefetch": 2,
       "warmup": 1, "repeats": 3, "runs": []}
for name, pred in ARMS:
    one_pass(pred)
    passes = [one_pass(pred) for _ in range(3)]
    out["runs"].append({"arm": name, "rows_kept": passes[0][1], "d2h_bytes": passes[0][2], "ms_best": round(min(p[0] for p in passes) * 1e3, 1),
                        "ms_all": [round(p[0] * 1e3, 1) for p in passes]})
    print(out["runs"][-1], file=sys.stderr, flush=True)
base = out["runs"][0]
out["vs_unfiltered"] = {r["arm"]: {"time": round(r["ms_best"] / base["ms_best"], 3), "d2h_bytes": round(r["d2h_bytes"] / base["d2h_bytes"], 4)} for r in out["runs"][1:]}
with open(out_path, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
