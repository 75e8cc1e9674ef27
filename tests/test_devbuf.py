"""Ownership rules of csrc/devbuf.h's Buf (the type behind every device and pinned buffer of the library), checked on
the CPU: tests/cpp/devbuf_test.cpp instantiates it with a counting malloc policy and runs under the address and
undefined-behaviour sanitizers.  No HIP, no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_buf_ownership_under_sanitizers(tmp_path):
    exe = str(tmp_path / "devbuf_test")
    subprocess.check_call(
        ["g++", "-std=c++20", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
         "-g", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "lsqrrecipes_amd", "csrc"),
         "-o", exe, os.path.join(ROOT, "tests", "cpp", "devbuf_test.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "devbuf test ok: live allocations 0" in r.stdout, r.stdout[-4000:]
