"""Rate of the GPU writer (orcgpu_writer_*, ArrowWriterBuilder): a 16-column lineitem-shaped table (numpy-generated) written to a
memory sink from host batches and from device-resident batches (the same columns in device memory, ORCGPU_ENC_ON_DEVICE), at the
default stripe size and at 4 MiB; beside it pyarrow.orc.write_table(..., compression="uncompressed") on the same table on the same
host (Apache ORC C++, the CPU baseline).  GB/s = Arrow bytes of the table in / wall seconds of the whole write (open .. close).
Usage: python profiles/writer_rate.py [rows]  -> one JSON object on stdout.

--compression snappy|lz4: the writer compresses every stream on the device (ArrowWriterBuilder.with_compression), at the default
64 MiB stripes; the file sizes are set against the uncompressed file and against pyarrow.orc.write_table(..., compression=...).
--kernel-stats FILE: folds in the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of the same command (the compression
kernels, lzc_*, against the writer's other device work).
--row-index-stride N: the writer with ROW_INDEX streams and statistics (ArrowWriterBuilder.with_row_index_stride) against the same
writes without them, uncompressed and with Snappy; with --kernel-stats, the row index kernels' (ix_*) share of the device time.
--types: the lineitem table with Decimal128(15,2) for its four money columns and Timestamp(ns) for l_shipdate, beside the stand-in
table of floats and integers in the same run (host batches, 64 MiB stripes, best of 3) and their ratio; with --kernel-stats, the
share of the Timestamp / Decimal128 kernels (wr_timestamp_kernel, wr_dec_*, wr_fill16_kernel) in the device time
(profiles/writer_rate_types.json).
--nested: a table of list<float32> (16 a row), a struct of three lineitem columns and a map<string,int64> (2 entries a row),
beside a flat table holding exactly the same leaf values (16 float columns, the three columns, two key and two value columns) in
the same run: the yardstick.  Twice: without nulls (every child column is a slice of its array) and with 5 % null lists / structs /
maps that keep their ranges (every child column is gathered through a row map).  GB/s of the leaf arrays' Arrow bytes; with
--kernel-stats the share of the flattening kernels (nest_*) in the device time (profiles/writer_rate_nested.json).
--dictionary T: the lineitem table written with ArrowWriterBuilder.with_dictionary_key_size_threshold(T) and, in the same run,
with threshold 0 (the yardstick: the writer as it is without dictionaries), host batches, 64 MiB stripes, best of 3: rows per
second, file sizes and their ratios; with --kernel-stats the share of the dictionary kernels (wd_*) in the device time
(profiles/writer_rate_dict.json).
--bloom-filter COLS (comma separated): the lineitem table written with ArrowWriterBuilder.with_bloom_filter_columns(COLS, fpp=0.01)
and, in the same run, with the row index alone (the yardstick), at --row-index-stride (10000 when not given), host batches, 64 MiB
stripes, best of 3: rows per second both ways, the file sizes; with --kernel-stats the share of the Bloom kernels (bloom_*) in the
device time.  Also written to profiles/writer_rate_bloom.json."""
import argparse
import csv
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np
import pyarrow as pa
import pyarrow.orc as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from orc_rust_amd import ArrowWriterBuilder, capi  # noqa: E402


class _ArrowArray(C.Structure):
    pass


_ArrowArray._fields_ = [("length", C.c_int64), ("null_count", C.c_int64), ("offset", C.c_int64), ("n_buffers", C.c_int64),
                        ("n_children", C.c_int64), ("buffers", C.POINTER(C.c_void_p)), ("children", C.POINTER(C.POINTER(_ArrowArray))),
                        ("dictionary", C.c_void_p), ("release", C.c_void_p), ("private_data", C.c_void_p)]


def lineitem(n, rng):
    def one(a):
        return a.combine_chunks() if isinstance(a, pa.ChunkedArray) else a
    cols = {
        "l_orderkey": np.repeat(np.arange(n // 4 + 1, dtype=np.int64) * 4, 4)[:n],
        "l_partkey": rng.integers(1, 200000, n).astype(np.int64),
        "l_suppkey": rng.integers(1, 10000, n).astype(np.int64),
        "l_linenumber": (np.arange(n) % 7 + 1).astype(np.int32),
        "l_quantity": rng.integers(1, 51, n).astype(np.float64),
        "l_extendedprice": np.round(rng.random(n) * 100000, 2),
        "l_discount": rng.integers(0, 11, n) / 100.0,
        "l_tax": rng.integers(0, 9, n) / 100.0,
        "l_returnflag": np.array(["A", "N", "R"])[rng.integers(0, 3, n)],
        "l_linestatus": np.array(["O", "F"])[rng.integers(0, 2, n)],
        "l_shipdate": rng.integers(8000, 10600, n).astype(np.int32),
        "l_commitdate": rng.integers(8000, 10600, n).astype(np.int32),
        "l_receiptdate": rng.integers(8000, 10600, n).astype(np.int32),
        "l_shipinstruct": np.array(["DELIVER IN PERSON", "COLLECT COD", "NONE", "TAKE BACK RETURN"])[rng.integers(0, 4, n)],
        "l_shipmode": np.array(["AIR", "MAIL", "SHIP", "TRUCK", "RAIL", "FOB", "REG AIR"])[rng.integers(0, 7, n)],
        "l_comment": np.char.add("c", rng.integers(0, 1 << 40, n).astype("U16")),
    }
    return pa.RecordBatch.from_pydict({k: one(pa.array(v)) for k, v in cols.items()})


MONEY = ["l_quantity", "l_extendedprice", "l_discount", "l_tax"]


def decimal_from_cents(cents):
    """Decimal128(15, 2) of int64 hundredths, from its buffer (16 bytes a value, little endian, sign-extended)"""
    v = np.empty((len(cents), 2), dtype=np.int64)
    v[:, 0] = cents
    v[:, 1] = cents >> 63
    return pa.Array.from_buffers(pa.decimal128(15, 2), len(cents), [None, pa.py_buffer(v.tobytes())])


def lineitem_types(batch):
    """the same rows with the types TPC-H gives them: the money columns Decimal128(15,2), l_shipdate a Timestamp(ns)"""
    cols = []
    for name, col in zip(batch.schema.names, batch.columns):
        if name in MONEY:
            col = decimal_from_cents(np.round(col.to_numpy() * 100).astype(np.int64))
        elif name == "l_shipdate":
            col = pa.array(col.to_numpy().astype(np.int64) * 86400 * 10 ** 9 + 12345, type=pa.int64()).cast(pa.timestamp("ns"))
        cols.append(col)
    return pa.RecordBatch.from_arrays(cols, names=batch.schema.names)


class DeviceBatch:
    """The batch's buffers copied to device memory (hipMalloc through the HIP runtime the library uses) as an ArrowArray."""

    def __init__(self, batch):
        hip = C.CDLL("libamdhip64.so")
        self.hip, self.ptrs = hip, []
        kids = []
        self.keep = []
        for col in batch.columns:
            bufs = []
            for b in col.buffers():
                if b is None:
                    bufs.append(None)
                    continue
                p = C.c_void_p()
                assert hip.hipMalloc(C.byref(p), C.c_size_t(max(1, b.size))) == 0
                assert hip.hipMemcpy(p, C.c_void_p(b.address), C.c_size_t(b.size), 1) == 0  # hipMemcpyHostToDevice
                self.ptrs.append(p)
                bufs.append(p.value)
            arr = _ArrowArray()
            cb = (C.c_void_p * len(bufs))(*bufs)
            arr.length, arr.null_count, arr.offset, arr.n_buffers, arr.n_children, arr.buffers = len(col), col.null_count, col.offset, len(bufs), 0, cb
            self.keep += [arr, cb]
            kids.append(C.pointer(arr))
        self.kids = (C.POINTER(_ArrowArray) * len(kids))(*kids)
        self.rbufs = (C.c_void_p * 1)(None)
        self.root = _ArrowArray()
        r = self.root
        r.length, r.null_count, r.offset, r.n_buffers, r.n_children, r.buffers, r.children = batch.num_rows, 0, 0, 1, len(kids), self.rbufs, self.kids

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


def gpu_write(ctx, batches, schema, sbs, device=None, compression=None, stride=0, dictionary=0.0, bloom=()):
    out = io.BytesIO()
    t0 = time.perf_counter()
    w = (ArrowWriterBuilder(out, schema, ctx=ctx).with_stripe_byte_size(sbs).with_compression(compression).with_row_index_stride(stride)
         .with_dictionary_key_size_threshold(dictionary).with_bloom_filter_columns(list(bloom), fpp=0.01).try_build())
    if device is None:
        for b in batches:
            w.write(b)
    else:
        sbuf = (C.c_uint8 * 72)()
        schema._export_to_c(C.addressof(sbuf))
        for d in device:
            w.write_c(C.addressof(sbuf), C.addressof(d.root), capi.ENC_ON_DEVICE)
        C.cast(C.addressof(sbuf) + 56, C.POINTER(C.CFUNCTYPE(None, C.c_void_p)))[0](C.addressof(sbuf))
    w.close()
    dt = time.perf_counter() - t0
    st = w.stats()
    w.free()
    return dt, st, out.getbuffer().nbytes


def kernel_stats(path):
    """rocprofv3's kernel_stats.csv -> the compression kernels' time against the rest of the device work"""
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    lzc = {r["Name"].split("(")[0]: round(float(r["TotalDurationNs"]) / 1e6, 3) for r in rows if r["Name"].startswith("lzc_")}
    top = max(rows, key=lambda r: float(r["TotalDurationNs"]))
    return {"what": "rocprofv3 --kernel-trace --stats of this command, all runs", "all_kernels_ms": round(total / 1e6, 3),
            "compression_kernels_ms": lzc, "compression_share": round(sum(lzc.values()) * 1e6 / total, 4),
            "largest_kernel": {"name": top["Name"].split("(")[0], "ms": round(float(top["TotalDurationNs"]) / 1e6, 3)}}


def main_compressed(args):
    n, per_batch = args.rows, 1_000_000
    rng = np.random.default_rng(1)
    batches = [lineitem(per_batch, rng) for _ in range(max(1, n // per_batch))]
    table = batches[0]
    n = per_batch * len(batches)
    arrow_bytes = sum(b.nbytes for b in batches)
    ctx = capi.Context()
    out = {"rows": n, "columns": table.num_columns, "arrow_bytes": arrow_bytes, "compression": args.compression,
           "unit": "GB/s of Arrow input (open .. close)", "runs": {}}
    gpu_write(ctx, batches[:1], table.schema, 64 << 20, compression=args.compression)  # warm-up
    device = [DeviceBatch(b) for b in batches]
    for comp in [args.compression, None]:
        for src in ["host", "device"]:
            best = None
            for _ in range(3):
                r = gpu_write(ctx, batches, table.schema, 64 << 20, device if src == "device" else None, compression=comp)
                if best is None or r[0] < best[0]:
                    best = r
            dt, st, size = best
            out["runs"]["default 64 MiB, %s batches, %s" % (src, comp or "uncompressed")] = {
                "seconds": round(dt, 4), "GB/s": round(arrow_bytes / dt / 1e9, 3), "file_bytes": size, "stripes": st["stripes"],
                "stripe_round_trips_per_stripe": round(st["stripe_round_trips"] / max(1, st["stripes"]), 1)}
    for d in device:
        d.free()
    runs = out["runs"]
    key = "default 64 MiB, host batches, %s" % args.compression
    out["rate_vs_uncompressed"] = round(runs[key]["GB/s"] / runs["default 64 MiB, host batches, uncompressed"]["GB/s"], 3)
    tt = pa.Table.from_batches(batches)
    buf = io.BytesIO()
    t0 = time.perf_counter()
    po.write_table(tt, buf, compression=args.compression)
    dt = time.perf_counter() - t0
    size = runs[key]["file_bytes"]
    out["file_size"] = {"this": size, "uncompressed": runs["default 64 MiB, host batches, uncompressed"]["file_bytes"],
                        "pyarrow": buf.getbuffer().nbytes,
                        "smaller_than_uncompressed": round(runs["default 64 MiB, host batches, uncompressed"]["file_bytes"] / size, 3),
                        "vs_pyarrow": round(size / buf.getbuffer().nbytes, 3)}
    out["cpu_baseline"] = {"what": "pyarrow.orc.write_table(compression=%r), same host" % args.compression, "seconds": round(dt, 4),
                           "GB/s": round(arrow_bytes / dt / 1e9, 3)}
    if args.kernel_stats:
        out["kernels"] = kernel_stats(args.kernel_stats)
    print(json.dumps(out))


def main_indexed(args):
    n, per_batch = args.rows, 1_000_000
    rng = np.random.default_rng(1)
    batches = [lineitem(per_batch, rng) for _ in range(max(1, n // per_batch))]
    table = batches[0]
    n = per_batch * len(batches)
    arrow_bytes = sum(b.nbytes for b in batches)
    ctx = capi.Context()
    out = {"rows": n, "columns": table.num_columns, "arrow_bytes": arrow_bytes, "row_index_stride": args.row_index_stride,
           "unit": "GB/s of Arrow input (open .. close), host batches, 64 MiB stripes, best of 3", "runs": {}, "rate_vs_unindexed": {}}
    gpu_write(ctx, batches[:1], table.schema, 64 << 20, stride=args.row_index_stride)  # warm-up
    for comp in [None, "snappy"]:
        for stride in [args.row_index_stride, 0]:
            best = None
            for _ in range(3):
                r = gpu_write(ctx, batches, table.schema, 64 << 20, compression=comp, stride=stride)
                if best is None or r[0] < best[0]:
                    best = r
            dt, st, size = best
            out["runs"]["%s, %s" % (comp or "uncompressed", "stride %d" % stride if stride else "no index")] = {
                "seconds": round(dt, 4), "GB/s": round(arrow_bytes / dt / 1e9, 3), "file_bytes": size, "stripes": st["stripes"],
                "stripe_round_trips_per_stripe": round(st["stripe_round_trips"] / max(1, st["stripes"]), 1)}
        runs = out["runs"]
        c = comp or "uncompressed"
        out["rate_vs_unindexed"][c] = round(runs["%s, stride %d" % (c, args.row_index_stride)]["GB/s"] / runs["%s, no index" % c]["GB/s"], 3)
    if args.kernel_stats:
        rows = list(csv.DictReader(open(args.kernel_stats)))
        total = sum(float(r["TotalDurationNs"]) for r in rows)
        ix = {r["Name"].split("(")[0]: round(float(r["TotalDurationNs"]) / 1e6, 3) for r in rows if r["Name"].startswith("ix_")}
        out["kernels"] = {"what": "rocprofv3 --kernel-trace --stats of this command, all runs", "all_kernels_ms": round(total / 1e6, 3),
                          "row_index_kernels_ms": ix, "row_index_share": round(sum(ix.values()) * 1e6 / total, 4)}
    print(json.dumps(out))


TYPE_KERNELS = ("wr_timestamp_kernel", "wr_dec_lengths_kernel", "wr_dec_pack_kernel", "wr_fill16_kernel")


def main_types(args):
    n, per_batch = args.rows, 1_000_000
    rng = np.random.default_rng(1)
    plain = [lineitem(per_batch, rng) for _ in range(max(1, n // per_batch))]
    typed = [lineitem_types(b) for b in plain]
    ctx = capi.Context()
    out = {"rows": per_batch * len(plain), "columns": plain[0].num_columns,
           "unit": "GB/s of Arrow input (open .. close), host batches, 64 MiB stripes, best of 3", "runs": {}}
    for name, batches in [("floats and integers (the stand-in)", plain), ("Decimal128(15,2) x 4, Timestamp(ns)", typed)]:
        arrow_bytes = sum(b.nbytes for b in batches)
        gpu_write(ctx, batches[:1], batches[0].schema, 64 << 20)  # warm-up
        best = None
        for _ in range(3):
            r = gpu_write(ctx, batches, batches[0].schema, 64 << 20)
            if best is None or r[0] < best[0]:
                best = r
        dt, st, size = best
        out["runs"][name] = {"seconds": round(dt, 4), "arrow_bytes": arrow_bytes, "GB/s": round(arrow_bytes / dt / 1e9, 3),
                             "Mrows/s": round(out["rows"] / dt / 1e6, 2), "file_bytes": size, "stripes": st["stripes"],
                             "stripe_round_trips_per_stripe": round(st["stripe_round_trips"] / max(1, st["stripes"]), 1)}
    a, b = out["runs"]["floats and integers (the stand-in)"], out["runs"]["Decimal128(15,2) x 4, Timestamp(ns)"]
    out["types_vs_stand_in"] = {"GB/s": round(b["GB/s"] / a["GB/s"], 3), "Mrows/s": round(b["Mrows/s"] / a["Mrows/s"], 3)}
    if args.kernel_stats:
        rows = list(csv.DictReader(open(args.kernel_stats)))
        total = sum(float(r["TotalDurationNs"]) for r in rows)
        ms = {r["Name"].split("(")[0]: round(float(r["TotalDurationNs"]) / 1e6, 3) for r in rows}
        mine = {k: v for k, v in ms.items() if k in TYPE_KERNELS}
        top = sorted(ms.items(), key=lambda kv: -kv[1])[:6]
        out["kernels"] = {"what": "rocprofv3 --kernel-trace --stats of this command, both tables, all runs", "all_kernels_ms": round(total / 1e6, 3),
                          "type_kernels_ms": mine, "type_kernels_share": round(sum(mine.values()) * 1e6 / total, 4), "largest_kernels_ms": dict(top)}
    print(json.dumps(out))


def nested_and_flat(n, rng, nulls):
    """(nested batch, flat batch of the same leaf values, bytes of the leaf arrays)"""
    li = lineitem(n, rng)
    f = rng.random(n * 16).astype(np.float32)
    keys = pa.array(np.array(["color", "size", "weight", "k"])[rng.integers(0, 4, 2 * n)])
    vals = pa.array(rng.integers(0, 1 << 30, 2 * n).astype(np.int64))
    three = [li.column("l_quantity"), li.column("l_linenumber"), li.column("l_returnflag")]

    def validity():
        return pa.py_buffer(np.packbits(rng.random(n) >= nulls, bitorder="little").tobytes()) if nulls else None
    lst = pa.Array.from_buffers(pa.list_(pa.float32()), n, [validity(), pa.py_buffer((np.arange(n + 1, dtype=np.int32) * 16).tobytes())], children=[pa.array(f)])
    st = pa.Array.from_buffers(pa.struct([("q", pa.float64()), ("n", pa.int32()), ("r", pa.string())]), n, [validity()], children=three)
    mt = pa.map_(pa.string(), pa.int64())
    entries = pa.StructArray.from_arrays([keys, vals], fields=[mt.key_field, mt.item_field])
    mp = pa.Array.from_buffers(mt, n, [validity(), pa.py_buffer((np.arange(n + 1, dtype=np.int32) * 2).tobytes())], children=[entries])
    nested = pa.RecordBatch.from_arrays([lst, st, mp], names=["emb", "item", "attrs"])
    cols, names = [pa.array(np.ascontiguousarray(f.reshape(n, 16)[:, k])) for k in range(16)], ["f%d" % k for k in range(16)]
    cols += three + [keys.take(pa.array(np.arange(k, 2 * n, 2))) for k in (0, 1)] + [vals.take(pa.array(np.arange(k, 2 * n, 2))) for k in (0, 1)]
    names += ["q", "n", "r", "k0", "k1", "v0", "v1"]
    flat = pa.RecordBatch.from_arrays(cols, names=names)
    return nested, flat, f.nbytes + sum(c.nbytes for c in three) + keys.nbytes + vals.nbytes


def main_nested(args):
    per_batch = 1_000_000
    ctx = capi.Context()
    out = {"rows": per_batch * max(1, args.rows // per_batch), "unit": "GB/s of the leaf arrays' Arrow bytes (open .. close), host batches, 64 MiB stripes, best of 3",
           "runs": {}, "nested_vs_flat": {}}
    for label, nulls in [("no nulls (slices)", 0.0), ("5 % null parents (gathers)", 0.05)]:
        rng = np.random.default_rng(1)
        made = [nested_and_flat(per_batch, rng, nulls) for _ in range(max(1, args.rows // per_batch))]
        leaf_bytes = sum(m[2] for m in made)
        for name, batches in [("flat", [m[1] for m in made]), ("nested", [m[0] for m in made])]:
            gpu_write(ctx, batches[:1], batches[0].schema, 64 << 20)  # warm-up
            best = None
            for _ in range(3):
                r = gpu_write(ctx, batches, batches[0].schema, 64 << 20)
                if best is None or r[0] < best[0]:
                    best = r
            dt, st, size = best
            out["runs"]["%s, %s" % (name, label)] = {
                "seconds": round(dt, 4), "leaf_bytes": leaf_bytes, "GB/s": round(leaf_bytes / dt / 1e9, 3), "file_bytes": size, "stripes": st["stripes"],
                "stripe_round_trips_per_stripe": round(st["stripe_round_trips"] / max(1, st["stripes"]), 1),
                "nested_slices": st["nested_slices"], "nested_gathers": st["nested_gathers"]}
        out["nested_vs_flat"][label] = round(out["runs"]["nested, " + label]["GB/s"] / out["runs"]["flat, " + label]["GB/s"], 3)
    if args.kernel_stats:
        rows = list(csv.DictReader(open(args.kernel_stats)))
        total = sum(float(r["TotalDurationNs"]) for r in rows)
        ms = {r["Name"].split("(")[0]: round(float(r["TotalDurationNs"]) / 1e6, 3) for r in rows}
        mine = {k: v for k, v in ms.items() if "nest_" in k}
        out["kernels"] = {"what": "rocprofv3 --kernel-trace --stats of this command, all tables, all runs", "all_kernels_ms": round(total / 1e6, 3),
                          "nested_kernels_ms": mine, "nested_kernels_share": round(sum(mine.values()) * 1e6 / total, 4),
                          "largest_kernels_ms": dict(sorted(ms.items(), key=lambda kv: -kv[1])[:6])}
    print(json.dumps(out))


def main_dictionary(args):
    per_batch = 1_000_000
    rng = np.random.default_rng(1)
    batches = [lineitem(per_batch, rng) for _ in range(max(1, args.rows // per_batch))]
    schema = batches[0].schema
    n = per_batch * len(batches)
    arrow_bytes = sum(b.nbytes for b in batches)
    ctx = capi.Context()
    out = {"rows": n, "columns": len(schema), "arrow_bytes": arrow_bytes, "threshold": args.dictionary,
           "unit": "Mrows/s (open .. close), host batches, 64 MiB stripes, best of 3, both arms in one process", "runs": {}}
    for t in (args.dictionary, 0.0):
        gpu_write(ctx, batches[:1], schema, 64 << 20, dictionary=t)  # warm-up
    times = {args.dictionary: [], 0.0: []}
    kept = {}
    for _ in range(3):  # (the arms take turns)
        for t in (args.dictionary, 0.0):
            dt, st, size = gpu_write(ctx, batches, schema, 64 << 20, dictionary=t)
            times[t].append(dt)
            kept[t] = (st, size)
    for t, name in ((args.dictionary, "threshold %g" % args.dictionary), (0.0, "threshold 0 (the yardstick)")):
        st, size = kept[t]
        dt = min(times[t])
        out["runs"][name] = {"seconds": round(dt, 4), "seconds_all": [round(x, 4) for x in times[t]], "Mrows/s": round(n / dt / 1e6, 2),
                             "GB/s": round(arrow_bytes / dt / 1e9, 3), "file_bytes": size, "stripes": st["stripes"],
                             "stripe_round_trips_per_stripe": round(st["stripe_round_trips"] / max(1, st["stripes"]), 1)}
    a, b = out["runs"]["threshold %g" % args.dictionary], out["runs"]["threshold 0 (the yardstick)"]
    out["rate_vs_yardstick"] = round(a["Mrows/s"] / b["Mrows/s"], 3)
    out["mark"] = 0.8
    out["file_size_vs_yardstick"] = round(a["file_bytes"] / b["file_bytes"], 4)
    if args.kernel_stats:
        rows = list(csv.DictReader(open(args.kernel_stats)))
        total = sum(float(r["TotalDurationNs"]) for r in rows)
        ms = {r["Name"].split("(")[0]: round(float(r["TotalDurationNs"]) / 1e6, 3) for r in rows}
        mine = {k: v for k, v in ms.items() if k.startswith("wd_")}
        out["kernels"] = {"what": "rocprofv3 --kernel-trace --stats of this command, both arms, all runs", "all_kernels_ms": round(total / 1e6, 3),
                          "dictionary_kernels_ms": mine, "dictionary_kernels_share": round(sum(mine.values()) * 1e6 / total, 4),
                          "largest_kernels_ms": dict(sorted(ms.items(), key=lambda kv: -kv[1])[:6])}
    print(json.dumps(out))


def main_bloom(args):
    per_batch = 1_000_000
    rng = np.random.default_rng(1)
    batches = [lineitem(per_batch, rng) for _ in range(max(1, args.rows // per_batch))]
    schema = batches[0].schema
    n = per_batch * len(batches)
    arrow_bytes = sum(b.nbytes for b in batches)
    stride = args.row_index_stride or 10000
    cols = [c for c in args.bloom_filter.split(",") if c]
    ctx = capi.Context()
    out = {"rows": n, "columns": len(schema), "arrow_bytes": arrow_bytes, "row_index_stride": stride, "bloom_filter_columns": cols, "fpp": 0.01,
           "unit": "Mrows/s (open .. close), host batches, 64 MiB stripes, best of 3, both arms in one process", "runs": {}}
    arms = (("bloom filters", tuple(cols)), ("row index only (the yardstick)", ()))
    for _, bloom in arms:
        gpu_write(ctx, batches[:1], schema, 64 << 20, stride=stride, bloom=bloom)  # warm-up
    times, kept = {name: [] for name, _ in arms}, {}
    for _ in range(3):  # (the arms take turns)
        for name, bloom in arms:
            dt, st, size = gpu_write(ctx, batches, schema, 64 << 20, stride=stride, bloom=bloom)
            times[name].append(dt)
            kept[name] = (st, size)
    for name, _ in arms:
        st, size = kept[name]
        dt = min(times[name])
        out["runs"][name] = {"seconds": round(dt, 4), "seconds_all": [round(x, 4) for x in times[name]], "Mrows/s": round(n / dt / 1e6, 2),
                             "GB/s": round(arrow_bytes / dt / 1e9, 3), "file_bytes": size, "stripes": st["stripes"],
                             "stripe_round_trips_per_stripe": round(st["stripe_round_trips"] / max(1, st["stripes"]), 1)}
    a, b = out["runs"][arms[0][0]], out["runs"][arms[1][0]]
    out["rate_vs_yardstick"] = round(a["Mrows/s"] / b["Mrows/s"], 3)
    out["file_size_vs_yardstick"] = round(a["file_bytes"] / b["file_bytes"], 4)
    if args.kernel_stats:
        rows = list(csv.DictReader(open(args.kernel_stats)))
        total = sum(float(r["TotalDurationNs"]) for r in rows)
        ms = {r["Name"].split("(")[0]: round(float(r["TotalDurationNs"]) / 1e6, 3) for r in rows}
        mine = {k: v for k, v in ms.items() if k.startswith("bloom_")}
        out["kernels"] = {"what": "rocprofv3 --kernel-trace --stats of this command in a run of its own, both arms, all runs",
                          "all_kernels_ms": round(total / 1e6, 3), "bloom_kernels_ms": mine,
                          "bloom_kernels_share": round(sum(mine.values()) * 1e6 / total, 4),
                          "largest_kernels_ms": dict(sorted(ms.items(), key=lambda kv: -kv[1])[:6])}
    text = json.dumps(out)
    with open(os.path.join(ROOT, "profiles", "writer_rate_bloom.json"), "w") as f:
        f.write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rows", nargs="?", type=int, default=8_000_000)
    ap.add_argument("--compression", choices=["snappy", "lz4"])
    ap.add_argument("--kernel-stats")
    ap.add_argument("--row-index-stride", type=int, default=0)
    ap.add_argument("--types", action="store_true")
    ap.add_argument("--nested", action="store_true")
    ap.add_argument("--dictionary", type=float, default=0.0)
    ap.add_argument("--bloom-filter", default="")
    args = ap.parse_args()
    if args.bloom_filter:
        return main_bloom(args)
    if args.dictionary:
        return main_dictionary(args)
    if args.nested:
        return main_nested(args)
    if args.types:
        return main_types(args)
    if args.row_index_stride:
        return main_indexed(args)
    if args.compression:
        return main_compressed(args)
    n = args.rows
    per_batch = 1_000_000
    rng = np.random.default_rng(1)
    batches = [lineitem(per_batch, rng) for _ in range(max(1, n // per_batch))]  # (each its own buffers: the device copies hold no more)
    table = batches[0]
    n = per_batch * len(batches)
    arrow_bytes = sum(b.nbytes for b in batches)
    ctx = capi.Context()
    out = {"rows": n, "columns": table.num_columns, "arrow_bytes": arrow_bytes, "unit": "GB/s of Arrow input (open .. close)", "runs": {}}
    gpu_write(ctx, batches[:1], table.schema, 64 << 20)  # warm-up (kernels loaded, buffers grown)
    device = [DeviceBatch(b) for b in batches]
    for sbs_name, sbs in [("default 64 MiB", 64 << 20), ("4 MiB", 4 << 20)]:
        for src in ["host", "device"]:
            best = None
            for _ in range(3):
                dt, st, size = gpu_write(ctx, batches, table.schema, sbs, device if src == "device" else None)
                if best is None or dt < best[0]:
                    best = (dt, st, size)
            dt, st, size = best
            out["runs"]["%s, %s batches" % (sbs_name, src)] = {
                "seconds": round(dt, 4), "GB/s": round(arrow_bytes / dt / 1e9, 3), "file_bytes": size, "stripes": st["stripes"],
                "round_trips": st["round_trips"], "round_trips_per_stripe": round(st["round_trips"] / max(1, st["stripes"]), 1),
                "stripe_round_trips_per_stripe": round(st["stripe_round_trips"] / max(1, st["stripes"]), 1)}
    for d in device:
        d.free()
    # the reference's usual pattern: many small writes into one stripe (the size analysis runs only near the stripe's limit)
    for rows_per_write in [8192, 1024]:
        small = [b.slice(i, rows_per_write) for b in batches for i in range(0, b.num_rows, rows_per_write)]
        dt, st, size = gpu_write(ctx, small, table.schema, 64 << 20)
        out["runs"]["default 64 MiB, host batches of %d rows" % rows_per_write] = {
            "seconds": round(dt, 4), "GB/s": round(arrow_bytes / dt / 1e9, 3), "file_bytes": size, "stripes": st["stripes"], "writes": len(small),
            "round_trips": st["round_trips"], "round_trips_per_write": round(st["round_trips"] / len(small), 2),
            "stripe_round_trips_per_stripe": round(st["stripe_round_trips"] / max(1, st["stripes"]), 1)}
    tt = pa.Table.from_batches(batches)
    best = None
    for _ in range(3):
        buf = io.BytesIO()
        t0 = time.perf_counter()
        po.write_table(tt, buf, compression="uncompressed")
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    out["cpu_baseline"] = {"what": "pyarrow.orc.write_table(compression='uncompressed'), same host", "seconds": round(best, 4),
                           "GB/s": round(arrow_bytes / best / 1e9, 3), "file_bytes": buf.getbuffer().nbytes}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
