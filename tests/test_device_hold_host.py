"""Device-resident batches, the part that needs no GPU: the reference counting that keeps a decoded result alive and unchanged while
exported arrays and DLPack tensors view it (orc_rust_amd/csrc/device_hold.h -- the text liborcgpu.so is built from) as a stand-alone
program under AddressSanitizer + UBSan, and the layout of struct ArrowDeviceArray as a plain C program sees it in include/orcgpu.h.
Nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.fixture(scope="module")
def hold_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("device_hold") / "device_hold_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "device_hold_check.cpp")])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_a_result_is_freed_once_and_never_before_its_last_release(hold_check):
    """N arrays and M tensors released one by one, the owner letting go (the reader moving on, closing, a plain free) at every
    point of that: one free, after the last release; a held result is never in the spare list; then releases from eight threads
    racing with the reader's close.  ASan and UBSan stay silent."""
    assert hold_check.returncode == 0, (hold_check.stdout[-2000:], hold_check.stderr[-3000:])
    word, scenarios, checks = hold_check.stdout.split()
    # N = 1..3 arrays x M = 0..2 tensors x 4 ways the owner lets go x its N + M + 1 places among the releases
    assert word == "ok" and int(scenarios) == 4 * sum(n + m + 1 for n in (1, 2, 3) for m in (0, 1, 2)) and int(checks) > 5 * int(scenarios)
    assert "runtime error" not in hold_check.stderr and "AddressSanitizer" not in hold_check.stderr


def test_arrow_device_array_layout_in_the_c_header(tmp_path):
    exe = str(tmp_path / "device_abi_check")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-o", exe, os.path.join(ROOT, "tests", "hostcheck", "device_abi_check.c")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout
