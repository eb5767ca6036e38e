"""DeviceRecordBatch / DeviceColumn: a batch of the GPU reader that stays in HBM (ArrowReaderBuilder.with_device_output()).

The batch is an Arrow C Device Data Interface array (`orcgpu_reader_next_batch_device`); its columns' buffers come out as torch
tensors on the context's device, zero-copy through DLPack (`orcgpu_device_array_dlpack`) -- but for what torch has no type for:
validity and Boolean values are bitmaps, unpacked to torch.bool by a kernel (`orcgpu_unpack_bits`).

    reader = ArrowReaderBuilder.try_new("file.orc").with_device_output().build()
    for batch in reader:                      # DeviceRecordBatch
        x = batch.column("l_quantity").values # torch.int64 on cuda:0, the decoder's own buffer
        writer.write_device(batch)            # ... or straight back into an ORC file, without leaving the device

A tensor keeps the memory it views alive: it may outlive the batch and the reader, not the context.
"""
import ctypes as C
import weakref

from . import capi  # noqa: F401

ARROW_DEVICE_ROCM = 10
_DLTENSOR = b"dltensor"  # (the capsule keeps the pointer, not a copy)


class ArrowArrayStruct(C.Structure):
    pass


ArrowArrayStruct._fields_ = [("length", C.c_int64), ("null_count", C.c_int64), ("offset", C.c_int64), ("n_buffers", C.c_int64),
                             ("n_children", C.c_int64), ("buffers", C.POINTER(C.c_void_p)),
                             ("children", C.POINTER(C.POINTER(ArrowArrayStruct))), ("dictionary", C.c_void_p),
                             ("release", C.CFUNCTYPE(None, C.c_void_p)), ("private_data", C.c_void_p)]


class ArrowDeviceArrayStruct(C.Structure):
    _fields_ = [("array", ArrowArrayStruct), ("device_id", C.c_int64), ("device_type", C.c_int32), ("sync_event", C.c_void_p),
                ("reserved", C.c_int64 * 3)]


assert C.sizeof(ArrowDeviceArrayStruct) == 128


def _torch_stream():
    """torch's current stream as a hipStream_t (0: the default stream)"""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("torch sees no GPU: import torch before the first orc_rust_amd call loads liborcgpu.so "
                           "(torch finds the device only when its HIP runtime is the first one in the process)")
    return C.c_void_p(torch.cuda.current_stream().cuda_stream or None)


def unpack_bits(ctx, bits, n):
    """An LSB-first bitmap (a uint8 tensor on the context's device) -> torch.bool of n, by the library's kernel on torch's current stream."""
    import torch
    out = torch.empty(n, dtype=torch.uint8, device=bits.device)
    if n:
        ctx._check(ctx.L.orcgpu_unpack_bits(ctx.h, C.c_void_p(bits.data_ptr()), n, C.c_void_p(out.data_ptr()), _torch_stream()))
    return out.view(torch.bool)


def _value_dtype(t):
    """torch dtype of a fixed-width column's values (what an empty batch's tensor gets; DLPack says it otherwise)"""
    import pyarrow as pa
    import torch
    if pa.types.is_dictionary(t):  # (with_dictionary_columns: the int32 keys)
        return torch.int32
    for test, dtype in ((pa.types.is_int8, torch.int8), (pa.types.is_int16, torch.int16), (pa.types.is_int32, torch.int32),
                        (pa.types.is_date32, torch.int32), (pa.types.is_float32, torch.float32), (pa.types.is_float64, torch.float64)):
        if test(t):
            return dtype
    return torch.int64


class DeviceDictionary:
    """The dictionary of a dictionary column (ArrowReaderBuilder.with_dictionary_columns), one per stripe and shared by the
    stripe's batches: `offsets` (int32, entries + 1, from 0) and `data` (uint8) in Arrow Utf8 layout, views of the decoder's
    buffers.  Entry k is data[offsets[k]:offsets[k + 1]]."""

    def __init__(self, column):
        import torch
        self._column = column
        self.offsets = column._dict_buffer(3, torch.int32)
        self.data = column._dict_buffer(4, torch.uint8, int(self.offsets[-1]))
        self.num_entries = int(self.offsets.shape[0]) - 1

    def to_pyarrow(self):
        """A host copy as a pyarrow.StringArray"""
        import pyarrow as pa
        bufs = [None, pa.py_buffer(self.offsets.cpu().numpy().tobytes()), pa.py_buffer(self.data.cpu().numpy().tobytes())]
        return pa.Array.from_buffers(pa.string(), self.num_entries, bufs, null_count=0)


class DeviceColumn:
    """One column of a DeviceRecordBatch.  `values`, `validity_bits`, `offsets` and `data` are views of the decoder's buffers;
    `validity` and a Boolean column's `values` are unpacked copies."""

    def __init__(self, batch, index):
        self._batch, self._index = batch, index
        child = batch._array.array.children[index].contents
        self.num_rows = child.length
        self.null_count = child.null_count
        self.type = batch.schema.field(index).type
        self._cache = {}

    def _buffer(self, which, dtype):
        """buffer `which` of the column through DLPack.  The library makes no tensor over nothing: a batch without rows, or string
        data without bytes, is an empty tensor of the buffer's dtype and shape made here."""
        import pyarrow as pa
        import torch
        b = self._batch
        if b._array is None:
            raise ValueError("the batch has been released")
        if self.num_rows == 0 and not (self._is_var() and which == 1):
            shape = (0, 2) if which == 1 and pa.types.is_decimal(self.type) else (0,)
            return torch.empty(shape, dtype=dtype, device=b.device)
        out = C.c_void_p()
        rc = b._ctx.L.orcgpu_device_array_dlpack(C.byref(b._array), self._index, which, C.byref(out))
        if rc == 101 and which == 2 and self._is_var():  # (the column and the array are right -- its offsets came the same way: no bytes)
            return torch.empty(0, dtype=dtype, device=b.device)
        b._ctx._check(rc)
        cap = _capsule(out.value)
        try:
            return torch.from_dlpack(cap)
        except Exception:
            # a capsule torch did not take still owns the tensor, and with it a reference on the decoded stripe
            if _PyCapsule_IsValid(cap, _DLTENSOR):
                C.cast(out.value + 56, C.POINTER(C.CFUNCTYPE(None, C.c_void_p)))[0](out.value)  # DLManagedTensor::deleter
            raise

    def _dict_buffer(self, which, dtype, n_bytes=None):
        """buffer 3 (offsets) or 4 (bytes, n_bytes of them by the offsets) of the column's dictionary.  The library makes no tensor
        over nothing, so what the exported array itself says is not there is made here: one zero offset for a stripe that decoded
        no rows (the dictionary array has no offsets buffer), no bytes for a dictionary whose last offset is 0.  Every other
        refusal of the library is an error."""
        import torch
        b = self._batch
        if b._array is None:
            raise ValueError("the batch has been released")
        child = b._array.array.children[self._index].contents
        if not child.dictionary:
            raise ValueError("column %d carries no dictionary" % self._index)
        d = C.cast(child.dictionary, C.POINTER(ArrowArrayStruct)).contents
        if which == 3 and not d.buffers[1]:
            return torch.zeros(1, dtype=dtype, device=b.device)
        if which == 4 and n_bytes == 0:
            return torch.empty(0, dtype=dtype, device=b.device)
        out = C.c_void_p()
        rc = b._ctx.L.orcgpu_device_array_dlpack(C.byref(b._array), self._index, which, C.byref(out))
        b._ctx._check(rc)
        cap = _capsule(out.value)
        try:
            return torch.from_dlpack(cap)
        except Exception:
            if _PyCapsule_IsValid(cap, _DLTENSOR):
                C.cast(out.value + 56, C.POINTER(C.CFUNCTYPE(None, C.c_void_p)))[0](out.value)  # DLManagedTensor::deleter
            raise

    @property
    def dictionary(self):
        """A dictionary column's DeviceDictionary (its `values` are the int32 keys, 0 in null rows); None for every other column"""
        import pyarrow as pa
        if not pa.types.is_dictionary(self.type):
            return None
        return self._cached("dictionary", lambda: DeviceDictionary(self))

    def _cached(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def _is_var(self):
        import pyarrow as pa
        return pa.types.is_string(self.type) or pa.types.is_binary(self.type)

    @property
    def validity_bits(self):
        """The validity bitmap as the decoder left it (uint8, LSB first), or None when the batch has no null."""
        import torch
        if not self.null_count:
            return None
        return self._cached("validity_bits", lambda: self._buffer(0, torch.uint8))

    @property
    def validity(self):
        """torch.bool per row (True: valid), or None when the batch has no null."""
        if not self.null_count:
            return None
        return self._cached("validity", lambda: unpack_bits(self._batch._ctx, self.validity_bits, self.num_rows))

    @property
    def values(self):
        """Fixed-width columns: the values in their natural dtype (Timestamp: int64; Decimal128: int64 [n, 2], low word first;
        Boolean: torch.bool, unpacked).  None for Utf8 / Binary (see offsets, data)."""
        import pyarrow as pa
        import torch
        if self._is_var():
            return None
        if pa.types.is_boolean(self.type):
            return self._cached("values", lambda: unpack_bits(self._batch._ctx, self._buffer(1, torch.uint8), self.num_rows))
        return self._cached("values", lambda: self._buffer(1, _value_dtype(self.type)))

    @property
    def values_bits(self):
        """A Boolean column's values as the decoder left them: the bitmap (uint8, LSB first)"""
        import torch
        return self._cached("values_bits", lambda: self._buffer(1, torch.uint8))

    @property
    def offsets(self):
        """Utf8 / Binary: int32 of num_rows + 1, from 0 in every batch"""
        import torch
        return self._cached("offsets", lambda: self._buffer(1, torch.int32)) if self._is_var() else None

    @property
    def data(self):
        """Utf8 / Binary: the batch's bytes (uint8)"""
        import torch
        return self._cached("data", lambda: self._buffer(2, torch.uint8)) if self._is_var() else None

    def to_pyarrow(self):
        """A host copy as a pyarrow.Array"""
        import pyarrow as pa

        def host(t):
            return pa.py_buffer(t.cpu().numpy().tobytes()) if t is not None else None

        bufs = [host(self.validity_bits)]
        if pa.types.is_dictionary(self.type):
            keys = pa.Array.from_buffers(pa.int32(), self.num_rows, bufs + [host(self.values)], null_count=self.null_count)
            return pa.DictionaryArray.from_arrays(keys, self.dictionary.to_pyarrow())
        if self._is_var():
            bufs += [host(self.offsets), host(self.data)]
        elif pa.types.is_boolean(self.type):
            bufs.append(host(self.values_bits))
        else:
            bufs.append(host(self.values))
        return pa.Array.from_buffers(self.type, self.num_rows, bufs, null_count=self.null_count)


_PyCapsule_New = C.pythonapi.PyCapsule_New
_PyCapsule_New.restype = C.py_object
_PyCapsule_New.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
_PyCapsule_IsValid = C.pythonapi.PyCapsule_IsValid
_PyCapsule_IsValid.restype = C.c_int
_PyCapsule_IsValid.argtypes = [C.py_object, C.c_char_p]


def _capsule(ptr):
    return _PyCapsule_New(ptr, _DLTENSOR, None)


class DeviceRecordBatch:
    """A record batch in HBM.  Constructed by the reader; `array` is the exported struct ArrowDeviceArray, which the batch owns
    and releases (release(), or when it is collected)."""

    def __init__(self, ctx, array, schema, reader=None):
        self._ctx, self._array, self.schema = ctx, array, schema
        self._reader = weakref.ref(reader) if reader is not None else None  # (write_device asks it whether its threads own the context)
        self.num_rows = array.array.length
        self.device_id = array.device_id
        if array.device_type != ARROW_DEVICE_ROCM:
            raise ValueError("not a ROCm device array (device_type %d)" % array.device_type)
        # whatever the caller enqueues on torch's current stream from here on runs behind the decode of this batch
        ctx._check(ctx.L.orcgpu_device_array_wait(C.byref(array), _torch_stream()))

    @property
    def device(self):
        import torch
        return torch.device("cuda", self.device_id)

    @property
    def num_columns(self):
        return len(self.schema)

    def column(self, i):
        if self._array is None:
            raise ValueError("the batch has been released")
        if isinstance(i, str):
            i = self.schema.get_field_index(i)
            if i < 0:
                raise KeyError("no such column")
        if not 0 <= i < self.num_columns:
            raise IndexError("column %d of %d" % (i, self.num_columns))
        return DeviceColumn(self, i)  # (it keeps the batch alive, not the other way round: no cycle for the collector to find)

    def to_pyarrow(self):
        """Copies the batch back: the pyarrow.RecordBatch the host path yields"""
        import pyarrow as pa
        return pa.RecordBatch.from_arrays([self.column(i).to_pyarrow() for i in range(self.num_columns)], schema=self.schema)

    def release(self):
        """Gives the batch's reference on the decoder's memory back.  Tensors taken from it stay valid: they hold their own."""
        a, self._array = self._array, None
        if a is not None and a.array.release:
            a.array.release(C.addressof(a))

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass
