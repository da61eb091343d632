"""csrc/foto_hostpool.h (the GN plan's host copy pool) under the host sanitizers: the stand-alone
tests/cpp/hostpool_check.cpp built with the host compiler, once with -fsanitize=thread and once
with -fsanitize=address,undefined, and run as a plain executable.  No GPU, nothing loaded into
Python, nothing preloaded."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "optical-flow-optimal-transport_amd", "csrc")
SRC = os.path.join(HERE, "cpp", "hostpool_check.cpp")


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if cxx and shutil.which(cxx):
            return cxx
    return None


@pytest.mark.parametrize("san", ["thread", "address,undefined"])
def test_hostpool_under_sanitizer(san, tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "hostpool_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", f"-fsanitize={san}", "-fno-sanitize-recover=all",
           "-I", CSRC, SRC, "-o", exe, "-pthread"]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0:
        # a compiler without this sanitizer's runtime fails at the link; anything else is a real error
        probe = subprocess.run([cxx, f"-fsanitize={san}", "-x", "c++", "-", "-o", str(tmp_path / "probe"), "-pthread"],
                               input="int main() { return 0; }\n", capture_output=True, text=True)
        if probe.returncode != 0:
            pytest.skip(f"{cxx}: no -fsanitize={san} runtime")
        pytest.fail(f"build failed:\n{b.stderr[-4000:]}")
    if os.environ.get("LD_PRELOAD") or (os.path.exists("/etc/ld.so.preload") and os.path.getsize("/etc/ld.so.preload")):
        pytest.skip("this host preloads a library into every process: a sanitizer's runtime must come first")
    env = dict(os.environ)
    env["TSAN_OPTIONS"] = "halt_on_error=1 exitcode=66"
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    print(r.stdout, r.stderr[-4000:])
    if r.returncode != 0 and "FATAL: ThreadSanitizer: unexpected memory mapping" in r.stderr:
        pytest.skip("ThreadSanitizer cannot map its shadow memory on this kernel")
    assert r.returncode == 0, r.stderr[-4000:]
    assert "hostpool_check ok" in r.stdout
    assert "Sanitizer" not in r.stderr
