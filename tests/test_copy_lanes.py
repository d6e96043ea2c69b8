"""Copy lanes (ops/csrc/copylanes.h): the lane of a window, the windows whose completion events
``h2d_done(k)`` consults, and the host-side "copied up to" account, which needs no device -- a
stand-alone program walks it over 1 and 2 lanes, 2..6 buffers and a few hundred windows under every
completion order of the windows in flight, built with AddressSanitizer + UBSan.
tests/test_copy_lanes_gpu.py holds the engine with two lanes against the engine with one."""

import os
import shutil
import subprocess

import pytest


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.timeout(300)
def test_copy_lane_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "llm_slo_ebpf_toolkit_amd", "ops", "csrc")
    exe = tmp_path / "copylanes_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-Wall", "-Werror", f"-I{csrc}", os.path.join(root, "tests", "native", "copylanes_host_check.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "copylanes host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
