"""Step lane (ops/csrc/steplane_host.h): what every side tracker's step shares before it touches the GPU
needs no device -- the span ranges of a step (``plan_ranges``: the three refusals' exact texts under each
of the eleven trackers' names, empty ranges skipped, exactly ``span_cap`` and one over) and the result
slots (``SlotRing``: before any step, negative indices, across the wrap, the exact message). A stand-alone
program walks them, built with AddressSanitizer + UBSan.
tests/test_steplane_gpu.py holds the slot reuse of every tracker on the device against its oracle."""

import os
import shutil
import subprocess

import pytest


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.timeout(300)
def test_step_lane_host_side_under_address_and_ub_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "llm_slo_ebpf_toolkit_amd", "ops", "csrc")
    exe = tmp_path / "steplane_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-Wall", "-Werror", f"-I{csrc}", os.path.join(root, "tests", "native", "steplane_host_check.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "steplane host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
