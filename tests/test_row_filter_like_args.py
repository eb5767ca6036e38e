"""The Python side of the LIKE leaf (orc_rust_amd/predicate.py): the constructors, what flatten() makes of a LIKE node (op 16, the
escape in `i`, the NULL pattern), the ValueErrors, and the escaping of starts_with / ends_with / contains.  No GPU."""
import ctypes as C

import pytest

import like_model as LM
from orc_rust_amd import predicate as PR
from orc_rust_amd.predicate import Predicate as P, PredicateValue as V


def node_bytes(n):
    # (the field's raw pointer: reading `n.s` would give a copy that ends at the first NUL)
    at = C.c_void_p.from_buffer(n, PR.PredicateNode.s.offset).value
    return C.string_at(at, n.s_len) if n.s_len else b""


def test_like_flattens_to_op_16_with_the_escape_in_i():
    assert PR.LIKE == 16 and PR.NOT == 10
    nodes, keep = P.like("l_comment", "%special%requests%").flatten()
    assert len(nodes) == 1
    n = nodes[0]
    assert (n.op, n.n_children, n.column, n.value_type, n.value_is_null, n.i) == (16, 0, b"l_comment", PR.PV_UTF8, 0, 0)
    assert node_bytes(n) == b"%special%requests%"
    nodes, keep = P.like("s", "hé_%", escape="!").flatten()  # (`keep` owns the bytes the nodes point to)
    n = nodes[0]
    assert n.i == ord("!") and node_bytes(n) == "hé_%".encode()
    nodes, keep = P.like("s", b"\xff%\x00_", escape="\\").flatten()  # bytes go through as they are, a NUL included
    n = nodes[0]
    assert n.i == 0x5C and n.s_len == 4 and node_bytes(n) == b"\xff%\x00_"
    nodes, keep = P.like("s", "").flatten()
    n = nodes[0]
    assert (n.value_is_null, n.s_len, n.i) == (0, 0, 0)


def test_the_null_pattern_and_not_like():
    nodes, keep = P.like("s", None, escape="#").flatten()
    n = nodes[0]
    assert (n.op, n.value_type, n.value_is_null, n.s_len, n.i) == (16, PR.PV_UTF8, 1, 0, ord("#"))
    nodes, _ = P.not_like("s", "a%", escape="\\").flatten()
    assert [x.op for x in nodes] == [PR.NOT, PR.LIKE] and nodes[0].n_children == 1 and nodes[1].i == 0x5C
    nodes, _ = P.and_([P.like("s", "a%"), P.or_([P.not_like("t", "%b"), P.eq("v", V.Int64(3))])]).flatten()
    assert [x.op for x in nodes] == [PR.AND, PR.LIKE, PR.OR, PR.NOT, PR.LIKE, PR.EQ]
    assert [x.i for x in nodes] == [0, 0, 0, 0, 0, 3]  # a comparison's literal is not disturbed


def test_value_errors():
    for bad in ("", "ab", "é", "\x00", 5, b"\\", ["!"]):
        with pytest.raises(ValueError):
            P.like("s", "a%", escape=bad)
    for bad in (5, 1.5, ["a"], V.Utf8("a")):
        with pytest.raises(ValueError):
            P.like("s", bad)
    for esc in ("\\", "!", "\x7f", "\x01", None):
        P.like("s", "a%", escape=esc)


@pytest.mark.parametrize("text", ["abc", "100%", "a_b", "back\\slash", "%_\\", "", "héllo_%", b"raw\xff%_\\"])
def test_the_conveniences_escape_what_they_must(text):
    as_bytes = text if isinstance(text, bytes) else text.encode()
    for make, lead, trail in ((P.starts_with, False, True), (P.ends_with, True, False), (P.contains, True, True)):
        p = make("s", text)
        nodes, keep = p.flatten()
        n = nodes[0]
        assert n.op == 16 and n.i == 0x5C and p.escape == "\\"
        pattern = node_bytes(n)
        body = pattern[1 if lead else 0:len(pattern) - (1 if trail else 0)]
        assert pattern.startswith(b"%") == lead or not as_bytes
        # unescaped, the body is the text again, and nothing in it is a wildcard any more
        assert LM.literal_prefix(body, 0x5C) == (as_bytes, False)
        want = {P.starts_with: "prefix", P.ends_with: "suffix", P.contains: "contains"}[make] if as_bytes else "all"
        assert LM.classify(pattern, 0x5C) == want
    if isinstance(text, str):  # ... and the model matches what the names say
        values = [text, "x" + text, text + "x", "x" + text + "x", "", "x"]
        for make, rule in ((P.starts_with, str.startswith), (P.ends_with, str.endswith), (P.contains, lambda v, t: t in v)):
            p = make("s", text)
            assert LM.like_column(values, p.value.value, p.escape) == [rule(v, text) for v in values]
