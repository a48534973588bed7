"""The host-only headers of csrc/ under AddressSanitizer and UBSan: a stand-alone driver (a .cpp under tests/helpers/ with its own
main and its own set_error) is built with g++ alone and run as a program of its own -- nothing is preloaded, no HIP, no device."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "glomeruli_segmentation_amd", "csrc")


def run_sanitized_driver(tmp_path, source, ok_line, flags=()):
    """builds tests/helpers/<source> and runs it; skips where g++ or the sanitizer runtime is absent; the driver must end with
    status 0, print `ok_line` and leave no sanitizer report.  -> its stdout"""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = tmp_path / os.path.splitext(source)[0]
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *flags, "-I" + CSRC,
           os.path.join(REPO, "tests", "helpers", source), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and "sanitize" in built.stderr and ("cannot find" in built.stderr or "unrecognized" in built.stderr):
        pytest.skip("sanitizer runtime not available: " + built.stderr[-300:])
    assert built.returncode == 0, built.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=77", UBSAN_OPTIONS="halt_on_error=1:exitcode=78")
    res = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.returncode, res.stdout[-500:], res.stderr[-3000:])
    assert ok_line in res.stdout, res.stdout[-500:]
    for word in ("AddressSanitizer", "runtime error"):
        assert word not in res.stderr, res.stderr[-3000:]
    return res.stdout


def assert_no_hip(header):
    """a plain host compiler reads csrc/<header>: outside its comments it names no HIP"""
    with open(os.path.join(CSRC, header)) as fh:
        assert "hip" not in re.sub(r"//.*", "", fh.read()).lower(), header
