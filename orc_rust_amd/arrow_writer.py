"""ArrowWriterBuilder / ArrowWriter: the reference's writer API (src/arrow_writer.rs:34-156) over the C ABI
(`orcgpu_writer_*`).  Pure plumbing: batches go over through the Arrow C Data Interface, every stream is encoded on the GPU.

    w = ArrowWriterBuilder("out.orc", schema).with_batch_size(1024).with_stripe_byte_size(64 << 20).try_build()
    w = ArrowWriterBuilder("out.orc", schema).with_compression("snappy").try_build()   # or "lz4"; compressed on the GPU
    w = ArrowWriterBuilder("out.orc", schema).with_row_index_stride(10000).try_build()  # row index + statistics, on the GPU
    w = ArrowWriterBuilder("out.orc", schema).with_dictionary_key_size_threshold(0.8).try_build()  # string dictionaries, on the GPU
    w = ArrowWriterBuilder("out.orc", schema).with_row_index_stride(10000).with_bloom_filter_columns(["k"], fpp=0.01).try_build()
    w.write(batch)          # pyarrow.RecordBatch
    w.write_device(batch)   # device_batch.DeviceRecordBatch (ArrowReaderBuilder.with_device_output()): encoded from HBM, no host copy
    w.flush_stripe()
    w.close()

`sink` is a path, or a binary file object: that is fed from the library's memory sink after every write, flush and at close.
"""
import ctypes as C

from . import capi

DEFAULT_BATCH_SIZE = 1024            # arrow_writer.rs:49
DEFAULT_STRIPE_BYTE_SIZE = 64 << 20  # arrow_writer.rs:51
DEFAULT_COMPRESSION_BLOCK_SIZE = 262144  # compression.rs:31
MAX_COMPRESSION_BLOCK_SIZE = (1 << 23) - 1  # a chunk header holds len * 2 + 1 in 24 bits
MAX_ROW_INDEX_STRIDE = (1 << 31) - 1
DEFAULT_BLOOM_FILTER_FPP = 0.01  # (with stride 10000: 1498 words and 7 hash functions, the filters of Apache ORC's bloom_filter.orc)
COMPRESSIONS = {None: 0, "none": 0, "snappy": 2, "lz4": 4}  # the codecs the writer compresses with (capi.COMP)

_SCHEMA_BYTES, _ARRAY_BYTES, _RELEASE_AT = 72, 80, {72: 56, 80: 64}  # struct ArrowSchema / ArrowArray, offset of `release`


class _Exported:
    """A pyarrow object exported to a C struct, released on exit."""

    def __init__(self, size):
        self.buf = (C.c_uint8 * size)()
        self.size = size

    @property
    def addr(self):
        return C.addressof(self.buf)

    def release(self):
        release = C.cast(self.addr + _RELEASE_AT[self.size], C.POINTER(C.CFUNCTYPE(None, C.c_void_p)))[0]
        if release:
            release(self.addr)


def _export_schema(schema):
    s = _Exported(_SCHEMA_BYTES)
    schema._export_to_c(s.addr)
    return s


class ArrowWriterBuilder:
    def __init__(self, sink, schema, ctx=None):
        self._sink, self._schema, self._ctx = sink, schema, ctx
        self._batch_size, self._stripe_byte_size = DEFAULT_BATCH_SIZE, DEFAULT_STRIPE_BYTE_SIZE
        self._compression, self._block_size = 0, DEFAULT_COMPRESSION_BLOCK_SIZE
        self._row_index_stride = 0
        self._dictionary_threshold = 0.0
        self._bloom_columns, self._bloom_fpp = [], DEFAULT_BLOOM_FILTER_FPP

    def with_batch_size(self, n):
        self._batch_size = int(n)
        return self

    def with_stripe_byte_size(self, n):
        self._stripe_byte_size = int(n)
        return self

    def with_compression(self, codec, block_size=DEFAULT_COMPRESSION_BLOCK_SIZE):
        """codec: None / "none" (the default: the reference's uncompressed file), "snappy" or "lz4" -- every stream compressed on the
        GPU in chunks of at most block_size bytes"""
        if codec not in COMPRESSIONS:
            raise ValueError("compression must be one of None, 'none', 'snappy', 'lz4', not %r" % (codec,))
        block_size = int(block_size)
        if block_size <= 0 or block_size > MAX_COMPRESSION_BLOCK_SIZE:
            raise ValueError("block_size must be in 1 .. 2^23 - 1")
        self._compression, self._block_size = COMPRESSIONS[codec], block_size
        return self

    def with_row_index_stride(self, stride):
        """Rows per row group of the ROW_INDEX streams and statistics (0, the default: none, the reference's file; Apache ORC's
        writers use 10000).  The row groups' statistics and positions are computed on the GPU."""
        if isinstance(stride, bool) or not isinstance(stride, int) and not hasattr(stride, "__index__"):
            raise ValueError("row_index_stride must be an integer, not %r" % (stride,))
        stride = int(stride.__index__())
        if stride < 0 or stride > MAX_ROW_INDEX_STRIDE:
            raise ValueError("row_index_stride must be 0 (none) or in 1 .. 2^31 - 1")
        self._row_index_stride = stride
        return self

    def with_dictionary_key_size_threshold(self, t):
        """0 (the default): every string column DIRECT_V2, the reference's file.  t in (0, 1]: per stripe, a Utf8 / LargeUtf8 column
        whose distinct values are at most t times its non-null values is written DICTIONARY_V2, its dictionary built on the GPU
        in first-occurrence order (Apache ORC's dictionary_key_size_threshold)."""
        if isinstance(t, bool) or not isinstance(t, (int, float)):
            raise ValueError("dictionary_key_size_threshold must be a number, not %r" % (t,))
        t = float(t)
        if t != t or t < 0.0 or t > 1.0:
            raise ValueError("dictionary_key_size_threshold must be in 0 .. 1")
        self._dictionary_threshold = t
        return self

    def with_bloom_filter_columns(self, columns, fpp=DEFAULT_BLOOM_FILTER_FPP):
        """A BLOOM_FILTER_UTF8 stream per row group for the named top-level columns (integers, floats, strings, binaries), built on
        the GPU and sized as Apache ORC sizes it from the row index stride and fpp, the false positive probability in (0, 1).
        Needs with_row_index_stride(n > 0) by try_build.  An empty list: none (the default)."""
        if not isinstance(columns, list) or not all(isinstance(c, str) for c in columns):
            raise ValueError("bloom filter columns must be a list of str, not %r" % (columns,))
        if isinstance(fpp, bool) or not isinstance(fpp, (int, float)):
            raise ValueError("fpp must be a number, not %r" % (fpp,))
        fpp = float(fpp)
        if not 0.0 < fpp < 1.0:  # (NaN fails both)
            raise ValueError("fpp must be strictly between 0 and 1")
        self._bloom_columns, self._bloom_fpp = list(columns), fpp
        return self

    def try_build(self):
        if self._bloom_columns and not self._row_index_stride:
            raise ValueError("bloom filter columns need with_row_index_stride(n) with n > 0: there is a filter per row group")
        if self._batch_size <= 0 or self._batch_size >= 1 << 32:
            raise ValueError("batch_size must be in 1 .. 2^32 - 1")
        if self._stripe_byte_size <= 0:  # (the C ABI reads 0 as the default)
            raise ValueError("stripe_byte_size must be positive")
        ctx = self._ctx or capi.Context(0)
        opts = capi.WriterOpts(self._batch_size, 0, self._stripe_byte_size)
        s = _export_schema(self._schema)
        out = C.c_void_p()
        try:
            if isinstance(self._sink, (str, bytes)) or hasattr(self._sink, "__fspath__"):
                import os
                path = os.fsencode(self._sink)
                ctx._check(ctx.L.orcgpu_writer_open_file(ctx.h, path, s.addr, C.byref(opts), C.byref(out)))
                fobj = None
            else:
                ctx._check(ctx.L.orcgpu_writer_open_bytes(ctx.h, s.addr, C.byref(opts), C.byref(out)))
                fobj = self._sink
        finally:
            s.release()
        w = ArrowWriter(ctx, out.value, self._schema, fobj)
        try:
            if self._compression:
                ctx._check(ctx.L.orcgpu_writer_set_compression(out.value, self._compression, self._block_size))
            if self._row_index_stride:
                ctx._check(ctx.L.orcgpu_writer_set_row_index(out.value, self._row_index_stride))
            if self._dictionary_threshold:
                ctx._check(ctx.L.orcgpu_writer_set_dictionary(out.value, self._dictionary_threshold))
            if self._bloom_columns:
                names = (C.c_char_p * len(self._bloom_columns))(*[c.encode() for c in self._bloom_columns])
                ctx._check(ctx.L.orcgpu_writer_set_bloom_filter(out.value, names, len(names), self._bloom_fpp))
        except Exception:
            w.free()
            raise
        w._drain()
        return w


class ArrowWriter:
    def __init__(self, ctx, handle, schema, fobj):
        self._ctx, self._h, self.schema, self._fobj = ctx, handle, schema, fobj

    def _check(self, rc):
        self._ctx._check(rc)

    def _drain(self):
        if self._fobj is None or not self._h:
            return
        n = C.c_uint64()
        self._check(self._ctx.L.orcgpu_writer_take_bytes(self._h, None, 0, C.byref(n)))
        if n.value:
            buf = (C.c_uint8 * n.value)()
            self._check(self._ctx.L.orcgpu_writer_take_bytes(self._h, buf, n.value, C.byref(n)))
            self._fobj.write(bytes(buf))

    def write(self, batch):
        """ArrowWriter::write: a pyarrow.RecordBatch (its schema must equal the writer's)."""
        s = _export_schema(batch.schema)
        a = _Exported(_ARRAY_BYTES)
        try:
            batch._export_to_c(a.addr)
            try:
                self.write_c(s.addr, a.addr, 0)
            finally:
                a.release()
        finally:
            s.release()

    def write_c(self, schema_addr, array_addr, flags=0):
        """The C ABI call: an exported ArrowSchema / ArrowArray (flags capi.ENC_ON_DEVICE: device buffers)."""
        self._check(self._ctx.L.orcgpu_writer_write(self._h, schema_addr, array_addr, flags))
        self._drain()

    def write_device(self, batch):
        """A device_batch.DeviceRecordBatch, written from its device buffers (ORCGPU_ENC_ON_DEVICE): nothing of it crosses the link.
        The writer's context must be on the batch's device.  On the batch's own context the write runs behind the decode on the same
        stream -- which needs a reader that does not read ahead (with_prefetch(0)), or one that has ended: a reading-ahead reader's
        threads own their context.  On another context of the same device the host waits for the batch's event first."""
        if batch._array is None:
            raise ValueError("the batch has been released")
        if self._ctx.device != batch.device_id:
            raise ValueError("the batch lives on device %d, the writer's context on device %d" % (batch.device_id, self._ctx.device))
        if self._ctx is batch._ctx:
            reader = batch._reader() if batch._reader is not None else None
            if reader is not None and reader.reads_ahead():
                raise ValueError("the batch's reader reads ahead on this context: give the writer a context of its own, or build the reader with_prefetch(0)")
        else:
            self._check(self._ctx.L.orcgpu_device_array_wait(C.byref(batch._array), None))
        s = _export_schema(batch.schema)
        try:
            self.write_c(s.addr, C.addressof(batch._array), capi.ENC_ON_DEVICE)
        finally:
            s.release()

    def flush_stripe(self):
        self._check(self._ctx.L.orcgpu_writer_flush_stripe(self._h))
        self._drain()

    def close(self):
        """Writes the open stripe (if it holds rows) and the file's tail.  stats() stay readable until free()."""
        self._check(self._ctx.L.orcgpu_writer_close(self._h))
        self._drain()

    def stats(self):
        c = capi.WriterCounts()
        self._check(self._ctx.L.orcgpu_writer_stats(self._h, C.byref(c)))
        return {k: getattr(c, k) for k, _ in capi.WriterCounts._fields_}

    def dictionary_counts(self):
        """(string column, stripe) pairs written so far: {"dictionary": DICTIONARY_V2, "direct": DIRECT_V2}"""
        d, r = C.c_uint64(), C.c_uint64()
        self._check(self._ctx.L.orcgpu_writer_dictionary_counts(self._h, C.byref(d), C.byref(r)))
        return {"dictionary": d.value, "direct": r.value}

    def stripe_rows(self):
        n = self.stats()["stripes"]
        return [self._ctx.L.orcgpu_writer_stripe_rows(self._h, i) for i in range(n)]

    def free(self):
        if self._h:
            self._ctx.L.orcgpu_writer_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
