"""ArrowReaderBuilder.with_dictionary_columns: what is checked in Python before anything reaches the GPU, and the binding's
constants.  No GPU: the builder under test is made without a context or a reader handle."""
import pytest

from orc_rust_amd import capi
from orc_rust_amd.arrow_reader import ArrowReaderBuilder, check_dictionary_columns


class _Lib:
    def __init__(self):
        self.calls = []

    def orcgpu_reader_set_dictionary_columns(self, h, arr, n):
        self.calls.append([arr[i].decode() for i in range(n)])
        return 0

    def orcgpu_reader_close(self, h):
        return None


class _Ctx:
    def __init__(self):
        self.L = _Lib()

    def _check(self, rc):
        assert rc == 0


def make_builder():
    return ArrowReaderBuilder(_Ctx(), 1)


@pytest.mark.parametrize("bad", ["l_shipmode", None, 7, {"a"}, {"a": 1}, (n for n in ["a"]), [1], ["a", None], ["a", b"b"], [""], ["a", ""],
                                 ["a", "a"], ("a", "b", "a"), [["a"]]])
def test_arguments_that_are_refused(bad):
    b = make_builder()
    with pytest.raises(ValueError):
        b.with_dictionary_columns(bad)
    assert b._ctx.L.calls == []  # nothing reached the library
    with pytest.raises(ValueError):
        check_dictionary_columns(bad)


@pytest.mark.parametrize("good", [["a"], ("a", "b"), ["l_returnflag", "l_linestatus", "l_shipmode"], [], ["ü", "a b"]])
def test_arguments_that_pass_and_chaining(good):
    b = make_builder()
    assert b.with_dictionary_columns(good) is b
    assert b._ctx.L.calls == [list(good)]


def test_binding_constants_and_exports():
    for name in ("orcgpu_result_dictionary_view", "orcgpu_result_copy_dictionary", "orcgpu_reader_set_dictionary_columns"):
        assert name in capi.EXPORTS
    assert capi.ARROW_DICTIONARY_UTF8 == 27
    assert capi.ABI_VERSION == 4
