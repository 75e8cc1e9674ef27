"""The rules of csrc/options.h (every name, rule and default of lsqr_set_option), checked on the CPU:
tests/cpp/options_test.cpp sets every option to values around every bound through options_set and compares status,
stored value and message with expectations written out there.  It runs under the address and undefined-behaviour
sanitizers.  No HIP, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "options_test")
    subprocess.check_call(
        ["g++", "-std=c++20", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
         "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "lsqrrecipes_amd", "csrc"),
         "-o", exe, os.path.join(ROOT, "tests", "cpp", "options_test.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "options test ok: 53 options" in r.stdout, r.stdout[-4000:]
