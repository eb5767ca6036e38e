"""The Python arguments of the key sets, checked before anything reaches the GPU (no GPU here: every check must fire before a
context is opened or a handle is touched)."""
import pytest

from orc_rust_amd import KeySet
from orc_rust_amd.arrow_reader import ArrowReader, ArrowReaderBuilder
from orc_rust_amd.key_set import MAX_KEYS, SENTINEL, check_collect_args
from orc_rust_amd.predicate import IN_SET, NOT, Predicate as P


def bare(cls):
    """An object of the class that has no handle and no context: a check that lets an argument through fails on it loudly"""
    return object.__new__(cls)


@pytest.mark.parametrize("column", (None, 5, b"k", ["k"]))
def test_a_column_that_is_no_str_is_a_type_error(column):
    with pytest.raises(TypeError, match="column"):
        ArrowReaderBuilder.collect_keys(bare(ArrowReaderBuilder), column)
    with pytest.raises(TypeError, match="column"):
        check_collect_args(column, 1, None)
    with pytest.raises(TypeError, match="column"):
        P.in_set(column, None)


def test_an_empty_column_name_is_a_value_error():
    with pytest.raises(ValueError, match="empty"):
        ArrowReaderBuilder.collect_keys(bare(ArrowReaderBuilder), "")


@pytest.mark.parametrize("max_keys", (True, False, 1.0, "8", None))
def test_max_keys_that_is_no_int_is_a_type_error(max_keys):
    with pytest.raises(TypeError, match="max_keys"):
        ArrowReaderBuilder.collect_keys(bare(ArrowReaderBuilder), "k", max_keys=max_keys)
    with pytest.raises(TypeError, match="max_keys"):
        KeySet(None, max_keys)


@pytest.mark.parametrize("max_keys", (0, -1, MAX_KEYS + 1, 1 << 40))
def test_max_keys_out_of_range_is_a_value_error(max_keys):
    with pytest.raises(ValueError, match="max_keys"):
        ArrowReaderBuilder.collect_keys(bare(ArrowReaderBuilder), "k", max_keys=max_keys)
    with pytest.raises(ValueError, match="max_keys"):
        KeySet(None, max_keys)


def test_the_limits_themselves_pass_the_check():
    check_collect_args("k", 1, None)
    check_collect_args("k", MAX_KEYS, None)
    assert MAX_KEYS == 1 << 26 and SENTINEL == int.from_bytes(b"\x80" * 8, "little", signed=True)


@pytest.mark.parametrize("into", (5, "set", object(), [1, 2]))
def test_into_that_is_no_key_set_is_a_type_error(into):
    with pytest.raises(TypeError, match="KeySet"):
        ArrowReaderBuilder.collect_keys(bare(ArrowReaderBuilder), "k", into=into)
    with pytest.raises(TypeError, match="KeySet"):
        ArrowReader.collect_keys(bare(ArrowReader), "k", into)


@pytest.mark.parametrize("what", (None, 5, {1, 2}, [1, 2], "keys", frozenset()))
def test_in_set_takes_a_key_set_only(what):
    with pytest.raises(TypeError, match="KeySet"):
        P.in_set("k", what)
    with pytest.raises(TypeError, match="KeySet"):
        P.not_in_set("k", what)


def test_the_leaf_and_its_negation_have_the_shape_the_header_says():
    ks = bare(KeySet)       # (never flattened here: no id is asked of it)
    ks._h = None
    p = P.in_set("k", ks)
    assert (p.op, p.column, p.key_set, p.children) == (IN_SET, "k", ks, []) and IN_SET == 26
    q = P.not_in_set("k", ks)
    assert q.op == NOT and len(q.children) == 1 and q.children[0].op == IN_SET and q.children[0].key_set is ks
    with pytest.raises(ValueError, match="closed"):       # a closed set cannot be named
        p.flatten()
