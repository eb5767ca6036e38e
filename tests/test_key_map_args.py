"""The Python arguments of the key maps and lookup columns, checked before anything reaches the GPU (no GPU here: every check must
fire before a context is opened or a handle is touched)."""
import pytest

from orc_rust_amd import KeyMap, KeySet, capi
from orc_rust_amd.arrow_reader import ArrowReader, ArrowReaderBuilder
from orc_rust_amd.key_map import LOOKUP_MAX, LOOKUP_MAX_PAIRS, MAX_VALUES, check_collect_map_args, check_lookup_args
from orc_rust_amd.key_set import MAX_KEYS, check_collect_args
from orc_rust_amd.predicate import IN_SET, Predicate as P


def bare(cls):
    """An object of the class that has no handle and no context: a check that lets an argument through fails on it loudly"""
    return object.__new__(cls)


def sealed_map(values=("a", "b"), ctx=None):
    """A KeyMap as the checks see a sealed one, without a library behind it"""
    m = bare(KeyMap)
    m._h, m.ctx, m.max_keys, m.value_names = None, ctx, 16, list(values)
    m._info = capi.KeyMapInfo()
    return m


def open_map(values=None):
    m = sealed_map()
    m._info, m.value_names = None, values
    return m


@pytest.mark.parametrize("key", (None, 5, b"k", ["k"]))
def test_a_key_that_is_no_str_is_a_type_error(key):
    with pytest.raises(TypeError, match="key column"):
        ArrowReaderBuilder.collect_map(bare(ArrowReaderBuilder), key, ["v"])
    with pytest.raises(TypeError, match="key column"):
        ArrowReader.collect_map(bare(ArrowReader), key, ["v"], open_map())
    with pytest.raises(TypeError, match="probe key"):
        ArrowReaderBuilder.with_lookup_columns(bare(ArrowReaderBuilder), sealed_map(), key, {"x": "a"})


def test_an_empty_key_name_is_a_value_error():
    with pytest.raises(ValueError, match="empty key"):
        ArrowReaderBuilder.collect_map(bare(ArrowReaderBuilder), "", ["v"])
    with pytest.raises(ValueError, match="empty probe key"):
        check_lookup_args(sealed_map(), "", {"x": "a"})


@pytest.mark.parametrize("values", (None, "v", 5, {"v"}, {"v": 1}))
def test_values_that_are_no_list_are_a_type_error(values):
    with pytest.raises(TypeError, match="value columns are a list"):
        ArrowReaderBuilder.collect_map(bare(ArrowReaderBuilder), "k", values)


def test_the_value_list_is_checked_entry_by_entry():
    with pytest.raises(TypeError, match="a value column is a str"):
        check_collect_map_args("k", ["v", 5], 1, None)
    with pytest.raises(ValueError, match="empty value"):
        check_collect_map_args("k", ["v", ""], 1, None)
    with pytest.raises(ValueError, match="'v' is given twice"):
        check_collect_map_args("k", ["v", "w", "v"], 1, None)
    with pytest.raises(ValueError, match="no value column"):
        check_collect_map_args("k", [], 1, None)
    with pytest.raises(ValueError, match="9 value columns, at most 8"):
        check_collect_map_args("k", ["v%d" % i for i in range(9)], 1, None)
    assert check_collect_map_args("k", tuple("v%d" % i for i in range(8)), MAX_KEYS, None) == ["v%d" % i for i in range(8)] and MAX_VALUES == 8


@pytest.mark.parametrize("max_keys", (True, 1.0, "8", None))
def test_max_keys_that_is_no_int_is_a_type_error(max_keys):
    with pytest.raises(TypeError, match="max_keys"):
        ArrowReaderBuilder.collect_map(bare(ArrowReaderBuilder), "k", ["v"], max_keys=max_keys)
    with pytest.raises(TypeError, match="max_keys"):
        KeyMap(None, max_keys)


@pytest.mark.parametrize("max_keys", (0, -1, MAX_KEYS + 1))
def test_max_keys_out_of_range_is_a_value_error(max_keys):
    with pytest.raises(ValueError, match="max_keys"):
        ArrowReaderBuilder.collect_map(bare(ArrowReaderBuilder), "k", ["v"], max_keys=max_keys)
    with pytest.raises(ValueError, match="max_keys"):
        KeyMap(None, max_keys)


@pytest.mark.parametrize("into", (5, "map", object(), bare(KeySet)))
def test_into_that_is_no_key_map_is_a_type_error(into):
    with pytest.raises(TypeError, match="KeyMap"):
        ArrowReaderBuilder.collect_map(bare(ArrowReaderBuilder), "k", ["v"], into=into)


def test_into_must_be_open_and_hold_the_same_values():
    with pytest.raises(ValueError, match="sealed"):
        check_collect_map_args("k", ["a", "b"], 1, sealed_map())
    with pytest.raises(ValueError, match="holds the values"):
        check_collect_map_args("k", ["a"], 1, open_map(["a", "b"]))
    assert check_collect_map_args("k", ["a", "b"], 1, open_map(["a", "b"])) == ["a", "b"]
    assert check_collect_map_args("k", ["a"], 1, open_map(None)) == ["a"]


def test_a_map_is_no_target_of_collect_keys_and_a_set_stays_one():
    with pytest.raises(TypeError, match="KeyMap"):
        check_collect_args("k", 1, open_map())
    ks = bare(KeySet)
    ks._info = None
    check_collect_args("k", 1, ks)  # as before


@pytest.mark.parametrize("what", (None, 5, "map", bare(KeySet), {"a": 1}))
def test_lookup_takes_a_key_map_only(what):
    with pytest.raises(TypeError, match="KeyMap"):
        ArrowReaderBuilder.with_lookup_columns(bare(ArrowReaderBuilder), what, "k", {"x": "a"})


def test_lookup_refusals():
    m = sealed_map()
    with pytest.raises(ValueError, match="not sealed"):
        check_lookup_args(open_map(["a"]), "k", {"x": "a"})
    with pytest.raises(ValueError, match="another context"):
        check_lookup_args(m, "k", {"x": "a"}, ctx=object())
    for columns in (None, ["x"], [("x", "a")], "x"):
        with pytest.raises(TypeError, match="dict"):
            check_lookup_args(m, "k", columns)
    with pytest.raises(ValueError, match="no lookup column"):
        check_lookup_args(m, "k", {})
    with pytest.raises(TypeError, match="are str"):
        check_lookup_args(m, "k", {"x": 0})
    with pytest.raises(TypeError, match="are str"):
        check_lookup_args(m, "k", {5: "a"})
    with pytest.raises(ValueError, match="empty output"):
        check_lookup_args(m, "k", {"": "a"})
    with pytest.raises(ValueError, match="holds no value 'c'"):
        check_lookup_args(m, "k", {"x": "c"})
    first = check_lookup_args(m, "k", {"x": "a", "y": "b"})
    assert first == [(m, "k", "x", 0), (m, "k", "y", 1)]
    with pytest.raises(ValueError, match="given already"):
        check_lookup_args(m, "k", {"z": "a"}, so_far=first)
    with pytest.raises(ValueError, match="'x' is given twice"):
        check_lookup_args(m, "k2", {"x": "a"}, so_far=first)
    assert check_lookup_args(m, "k2", {"z": "a"}, so_far=first) == [(m, "k2", "z", 0)]  # the same map on another key: another pair


def test_lookup_limits():
    m = sealed_map(["v%d" % i for i in range(8)])
    eight = check_lookup_args(m, "k", {"o%d" % i: "v%d" % i for i in range(8)})
    assert len(eight) == LOOKUP_MAX == 8
    with pytest.raises(ValueError, match="9 lookup columns, at most 8"):
        check_lookup_args(m, "k2", {"p": "v0"}, so_far=eight)
    so_far = []
    for i in range(LOOKUP_MAX_PAIRS):
        so_far += check_lookup_args(m, "k%d" % i, {"o%d" % i: "v0"}, so_far=so_far)
    with pytest.raises(ValueError, match="more than 4"):
        check_lookup_args(m, "k4", {"o4": "v0"}, so_far=so_far)


def test_a_sealed_map_is_named_by_in_set_as_a_set_is():
    m = sealed_map()
    p = P.in_set("k", m)
    assert (p.op, p.column, p.key_set) == (IN_SET, "k", m) and isinstance(m, KeySet)
    with pytest.raises(ValueError, match="closed"):
        p.flatten()


def test_the_builder_is_unchanged_when_neither_is_called():
    b = ArrowReaderBuilder(None, None)
    assert set(vars(b)) == {"_ctx", "_h", "_keep", "_device_output"}
    import orc_rust_amd
    assert orc_rust_amd.KeyMap is KeyMap and "KeyMap" in orc_rust_amd.__all__ and "KeySet" in orc_rust_amd.__all__
