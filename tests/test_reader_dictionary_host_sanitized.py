"""tests/hostcheck/dictionary_check.cpp under AddressSanitizer + UBSan: the name list of orcgpu_reader_set_dictionary_columns (the
library's own text, orc_rust_amd/csrc/orcgpu_dictionary_names.inc) and the reference-counting primitive (device_hold.h) that keeps a
stripe's shared dictionary alive until the last batch referring to it is released, in every release order -- the primitive only:
the export's release callbacks are HIP text and are exercised by the GPU tests.  A stand-alone program: no GPU, nothing
loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]


def test_dictionary_names_and_release_counting_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "dictionary_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-pthread"] + SAN + ["-o", exe, os.path.join(ROOT, "tests", "hostcheck", "dictionary_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "dictionary_check ok" in p.stdout
