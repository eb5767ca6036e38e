"""The computed columns' plan under AddressSanitizer + UBSan on the CPU: tests/hostcheck/computed_check.cpp compiles
orc_rust_amd/csrc/orcgpu_computed_plan.inc and device/agg_expr_eval.h -- the text liborcgpu.so is built from -- into a stand-alone
program.  The plan for each class, the program table's layout, the names against the file's roots, every refusal with its status
and message fragment; and the interpreter the kernel runs, driven over the hand cases of tests/test_computed_model.py with the
operands this test passes in, against tests/computed_model.py.  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

import computed_model as M
from orc_rust_amd.aggregate import col

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
OK, MISMATCHED, UNSUPPORTED, INVALID = 0, 6, 7, 101
INT, DEC, FLOAT = 0, 1, 2
SCHEMA = {"a": "int", "b": "int", "d": "date", "p": ("dec", 2), "q": ("dec", 10), "w": ("dec", 0), "x": "float", "y": "float"}
NAN, NEG_ZERO = float("nan"), -0.0
# (name, the expression for the program, the same for the model, the row)
EVALS = [
    ("max_plus_1", "+ c:a c:b", col("a") + col("b"), {"a": 2 ** 63 - 1, "b": 1}),
    ("max_plus_0", "+ c:a c:b", col("a") + col("b"), {"a": 2 ** 63 - 1, "b": 0}),
    ("min_minus_0", "- c:a c:b", col("a") - col("b"), {"a": -2 ** 63, "b": 0}),
    ("min_minus_1", "- c:a c:b", col("a") - col("b"), {"a": -2 ** 63, "b": 1}),
    ("neg_min", "neg c:a", -col("a"), {"a": -2 ** 63}),
    ("null_operand", "+ c:a c:b", col("a") + col("b"), {"a": 5, "b": None}),
    ("date_days", "- c:d c:a", col("d") - col("a"), {"d": 19000, "a": 7}),
    ("dec_2x2", "* c:p c:p", col("p") * col("p"), {"p": 150}),
    ("dec_exact_limit_minus_1", "+ c:w c:a", col("w") + col("a"), {"w": 10 ** 38 - 2, "a": 1}),
    ("dec_exact_limit", "+ c:w c:a", col("w") + col("a"), {"w": 10 ** 38 - 1, "a": 1}),
    ("dec_neg_limit", "- c:w c:a", col("w") - col("a"), {"w": 1 - 10 ** 38, "a": 1}),
    ("neg_neg_2_127", "neg * c:w c:p", -(col("w") * col("p")), {"w": -2 ** 64, "p": 2 ** 63}),  # -(-2^127) leaves 128 bits
    ("leaves_128_bits", "* c:w c:w", col("w") * col("w"), {"w": 2 ** 64}),
    ("tenth_plus_fifth", "+ c:x c:y", col("x") + col("y"), {"x": 0.1, "y": 0.2}),
    ("nan", "+ c:x c:y", col("x") + col("y"), {"x": NAN, "y": 1.0}),
    ("neg_zero_product", "* c:x c:y", col("x") * col("y"), {"x": NEG_ZERO, "y": 5.0}),
    ("zero_sum", "+ c:x c:y", col("x") + col("y"), {"x": NEG_ZERO, "y": 0.0}),
    ("no_contraction", "+ * c:x c:y f:0.5", col("x") * col("y") + 0.5, {"x": 0.1, "y": 0.30000000000000004}),
]


def operand(name, v):
    return "%s=%s" % (name, "%x" % M.bits(v) if SCHEMA[name] == "float" else str(v))


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("computed_host") / "computed_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "computed_check.cpp")])
    args = []
    for name, text, _, row in EVALS:
        args += ["eval", name, text] + [operand(k, v) for k, v in row.items() if v is not None]
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    got = {}
    for ln in run.stdout.splitlines():
        head, _, msg = ln.partition("\t")
        f = head.split()
        got[(f[0], f[1])] = (f[2:], msg)
    return got


def plan(out, name):
    """status, n columns, n ops, [(class, scale, first op, n ops, columns read)], message"""
    f, msg = out[("plan", name)]
    return int(f[0]), int(f[1]), int(f[2]), [tuple(int(x) for x in c.split(":")) for c in f[3:]], msg


def test_the_plan_for_each_class(out):
    assert plan(out, "int")[:4] == (OK, 1, 5, [(INT, 0, 0, 5, 2)])  # two gates, two pushes, the add
    assert plan(out, "date")[:4] == (OK, 1, 5, [(INT, 0, 0, 5, 2)])  # a Date is int64 days
    assert plan(out, "dec_2x2")[:4] == (OK, 1, 4, [(DEC, 4, 0, 4, 1)])  # scales 2 x 2 give 4; one gate for the column named twice
    assert plan(out, "dec_rev")[3] == [(DEC, 12, 0, 7, 2)]  # p * (1 - q): 2 + 10, the literal scaled into place
    assert plan(out, "float")[3] == [(FLOAT, 0, 0, 7, 2)]
    for name, e in (("int", col("a") + col("b")), ("dec_2x2", col("p") * col("p")), ("dec_rev", col("p") * (1 - col("q"))), ("float", col("x") * col("y") + 0.5)):
        kind, scale = M.output_type(e, SCHEMA)
        assert plan(out, name)[3][0][:2] == ({M.INT64: INT, M.DEC128: DEC, M.FLOAT64: FLOAT}[kind], scale), name


def test_the_program_table_is_laid_out_one_program_behind_the_other(out):
    status, n, n_ops, cols, _ = plan(out, "three")
    assert (status, n, n_ops) == (OK, 3, 13)
    assert cols == [(INT, 0, 0, 5, 2), (DEC, 12, 5, 5, 2), (FLOAT, 0, 10, 3, 1)]
    status, n, n_ops, cols, _ = plan(out, "eight")
    assert (status, n, n_ops) == (OK, 8, 32) and [c[2] for c in cols] == list(range(0, 32, 4))


def test_names_against_each_other_and_the_roots(out):
    for name, words in (("nine", "more than ORCGPU_COMPUTED_MAX (8)"), ("empty_name", "without a name"), ("twice", "the name 'r' is given twice"),
                        ("root_name", "'q' is the name of a root column of the file"), ("root_name_unprojected", "'st' is the name of a root column of the file")):
        status, _, _, _, msg = plan(out, name)
        assert status == INVALID and words in msg, (name, msg)
    assert M.check_names(["r", "r"], set(SCHEMA)) == "twice" and M.check_names(["q"], set(SCHEMA)) == "root" and M.check_names([""], set(SCHEMA)) == "empty"


def test_every_refusal_names_the_computed_column(out):
    for name, code, words in (("string", UNSUPPORTED, "column 's' cannot stand in the expression of computed column 'r'"),
                              ("boolean", UNSUPPORTED, "column 't' cannot stand in the expression of computed column 'r'"),
                              ("timestamp", UNSUPPORTED, "column 'ts' cannot stand in the expression of computed column 'r'"),
                              ("dictionary", UNSUPPORTED, "column 's' is read as a dictionary column: computed column 'r'"),
                              ("nested_projection", UNSUPPORTED, "the projected column 'st' is nested"),
                              ("computed_operand", UNSUPPORTED, "computed column 'u': its operand 'r' is a computed column"),
                              ("no_column", INVALID, "computed column 'r': its expression holds no column"),
                              ("unknown", INVALID, "column 'nope' in the expression of computed column 'r' is not a projected root column"),
                              ("mixed", MISMATCHED, "computed column 'r' mixes the Float / Double column 'x'"),
                              ("scale_40", UNSUPPORTED, "computed column 'r' over column 'q' has a scale of more than 38"),
                              ("no_nodes", INVALID, "computed column 'r' without an expression")):
        status, _, _, _, msg = plan(out, name)
        assert status == code and words in msg, (name, status, msg)


@pytest.mark.parametrize("case", EVALS, ids=[c[0] for c in EVALS])
def test_the_interpreter_on_the_hand_cases(out, case):
    name, _, e, row = case
    full = {k: row.get(k) for k in SCHEMA}
    want, over = M.eval_value(e, SCHEMA, full)
    f, _ = out[("eval", name)]
    state = int(f[0])
    assert state == (2 if over else 0 if want is None else 1), (name, f)
    if want is not None:
        kind, _ = M.output_type(e, SCHEMA)
        assert (int(f[1], 16) if kind == M.FLOAT64 else int(f[1])) == (M.bits(want) if kind == M.FLOAT64 else want), (name, f)


def test_the_hand_cases_hold_the_edges():
    want = {c[0]: M.eval_value(c[2], SCHEMA, {k: c[3].get(k) for k in SCHEMA}) for c in EVALS}
    assert want["max_plus_1"] == (None, True) and want["min_minus_0"] == (-2 ** 63, False) and want["neg_min"] == (None, True)
    assert want["dec_exact_limit_minus_1"] == (10 ** 38 - 1, False) and want["dec_exact_limit"] == (None, True) and want["dec_neg_limit"] == (None, True)
    assert want["dec_2x2"] == (22500, False) and want["null_operand"] == (None, False)
    assert want["neg_neg_2_127"] == (None, True)
    assert want["leaves_128_bits"] == (None, True)
    assert M.bits(want["tenth_plus_fifth"][0]) == 0x3FD3333333333334 and M.bits(want["neg_zero_product"][0]) == 1 << 63 and M.bits(want["zero_sum"][0]) == 0
