"""The device-output entry points of the C ABI where no GPU is needed: they refuse NULL arguments and arrays that are not theirs
before touching a device, and the binding and the library agree on the ABI version."""
import ctypes as C

from orc_rust_amd import capi
from orc_rust_amd.device_batch import ArrowDeviceArrayStruct

INVALID = 101


def test_abi_version_matches_the_binding():
    L = capi.load()
    assert L.orcgpu_abi_version() == capi.ABI_VERSION == 4


def test_null_arguments_are_invalid():
    L = capi.load()
    a = ArrowDeviceArrayStruct()
    s = (C.c_uint8 * 72)()
    n = C.c_uint64(7)
    out = C.c_void_p()
    buf = (C.c_uint8 * 64)()
    fake = C.c_void_p(C.addressof(buf))  # never dereferenced: the NULL argument is seen first
    assert L.orcgpu_result_export_batch_device(None, None, 0, C.addressof(a), C.addressof(s)) == INVALID
    assert L.orcgpu_result_export_batch_device(fake, None, 0, C.addressof(a), C.addressof(s)) == INVALID
    assert L.orcgpu_reader_set_device_output(None, 1) == INVALID
    assert L.orcgpu_reader_next_batch_device(None, C.addressof(a), C.addressof(s)) == INVALID
    assert L.orcgpu_reader_next_batch_device(fake, None, C.addressof(s)) == INVALID
    assert L.orcgpu_reader_d2h_bytes(None, C.byref(n)) == INVALID and n.value == 7
    assert L.orcgpu_reader_d2h_bytes(fake, None) == INVALID
    assert L.orcgpu_device_array_wait(None, None) == INVALID
    assert L.orcgpu_device_array_dlpack(None, 0, 1, C.byref(out)) == INVALID
    assert L.orcgpu_device_array_dlpack(C.addressof(a), 0, 1, None) == INVALID
    assert L.orcgpu_unpack_bits(None, fake, 8, fake, None) == INVALID


def test_arrays_of_another_producer_are_refused():
    """A released array (release == NULL) has no event to wait for and no buffers; an array whose release callback is not the
    library's own gets no DLPack tensor: its private data is somebody else's."""
    L = capi.load()
    a = ArrowDeviceArrayStruct()
    out = C.c_void_p(1)
    assert L.orcgpu_device_array_wait(C.addressof(a), None) == INVALID
    assert L.orcgpu_device_array_dlpack(C.addressof(a), 0, 1, C.byref(out)) == INVALID and out.value is None
    foreign = C.CFUNCTYPE(None, C.c_void_p)(lambda p: None)
    a.array.release = foreign
    a.array.private_data = C.addressof(a)
    a.device_type = 10
    assert L.orcgpu_device_array_dlpack(C.addressof(a), 0, 1, C.byref(out)) == INVALID
