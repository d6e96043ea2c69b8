"""Copy ahead on the host (ops/csrc/copylanes.h): the slots of the copy-side events, two buffer
counts deep, and the "copied up to" account when a window counts from its copy phase on -- a
stand-alone program walks the engine's protocol over one and two lanes (and a lane count that
changes in mid-run), 2..5 buffers and every completion order of
the windows in flight, built with AddressSanitizer + UBSan. tests/test_copy_ahead_gpu.py holds the
engine and the worker."""

import os
import shutil
import subprocess

import pytest


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.timeout(300)
def test_copy_ahead_arithmetic_under_address_and_ub_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "llm_slo_ebpf_toolkit_amd", "ops", "csrc")
    exe = tmp_path / "copyahead_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-Wall", "-Werror", f"-I{csrc}", os.path.join(root, "tests", "native", "copyahead_host_check.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "copyahead host ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_the_cpu_engine_keeps_the_plain_order():
    """No copy phase to issue early: the worker stages a window of the CPU engine in one piece."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    pipe = WindowPipeline(4096, 256, 8, model="bayes", learn=False, engine="cpu")
    assert not pipe.eng.copy_ahead and not pipe.copy_ahead
