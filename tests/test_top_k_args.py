"""Every TypeError and ValueError of orc_rust_amd/top_k.py: the arguments of with_top_k / top_k are checked before anything
reaches the GPU.  No GPU, no library."""
import pytest

from orc_rust_amd import top_k as T
from orc_rust_amd.top_k import SortKey


def test_sort_key_defaults_and_forms():
    k = SortKey("a")
    assert (k.column, k.descending, k.nulls_first) == ("a", False, False)
    assert T.as_key("a") == SortKey("a")
    assert T.as_key(("a", "desc")) == SortKey("a", descending=True)
    assert T.as_key(("a", "asc")) == SortKey("a")
    assert T.check_keys("a") == [SortKey("a")]
    assert T.check_keys(("a", "desc")) == [SortKey("a", descending=True)]
    assert T.check_keys(SortKey("a", nulls_first=True)) == [SortKey("a", nulls_first=True)]
    assert T.check_keys(["a", ("b", "desc"), SortKey("c", True, True)]) == [SortKey("a"), SortKey("b", True), SortKey("c", True, True)]
    assert T.check_keys(("a", "b")) == [SortKey("a"), SortKey("b")]          # a tuple of two names is two keys
    assert "desc" in repr(SortKey("a", True))


@pytest.mark.parametrize("args", [(1,), (None,), (b"a",), ("a", 1), ("a", "yes"), ("a", False, 0), ("a", None)])
def test_sort_key_type_errors(args):
    with pytest.raises(TypeError):
        SortKey(*args)


def test_sort_key_empty_name():
    with pytest.raises(ValueError):
        SortKey("")


@pytest.mark.parametrize("key", [1, None, 1.5, ["a"], {"a": "asc"}, ("a", 1), (1, "asc")])
def test_as_key_type_errors(key):
    with pytest.raises(TypeError):
        T.as_key(key)


@pytest.mark.parametrize("key", [("a", "up"), ("a", "DESC"), ("a",), ("a", "asc", "x"), ("", "asc")])
def test_as_key_value_errors(key):
    with pytest.raises(ValueError):
        T.as_key(key)


@pytest.mark.parametrize("by", [1, None, {"a"}, 2.5])
def test_check_keys_type_errors(by):
    with pytest.raises(TypeError):
        T.check_keys(by)


def test_check_keys_value_errors():
    with pytest.raises(ValueError, match="no sort key"):
        T.check_keys([])
    with pytest.raises(ValueError, match="at most 4"):
        T.check_keys(["a", "b", "c", "d", "e"])
    with pytest.raises(ValueError, match="listed twice"):
        T.check_keys(["a", ("a", "desc")])
    assert len(T.check_keys(["a", "b", "c", "d"])) == 4


@pytest.mark.parametrize("k", [True, False, 1.0, "1", None, [1]])
def test_check_k_type_errors(k):
    with pytest.raises(TypeError):
        T.check_k(k)


@pytest.mark.parametrize("k", [0, -1, 65537, 1 << 40])
def test_check_k_value_errors(k):
    with pytest.raises(ValueError):
        T.check_k(k)


def test_check_k_bounds_and_key_array():
    assert T.check_k(1) == 1 and T.check_k(65536) == 65536
    arr, keep = T.key_array([("x", "desc"), SortKey("y", nulls_first=True)])
    assert len(arr) == 2
    assert (arr[0].column, arr[0].descending, arr[0].nulls_first) == (b"x", 1, 0)
    assert (arr[1].column, arr[1].descending, arr[1].nulls_first) == (b"y", 0, 1)
