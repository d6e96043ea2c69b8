"""The step lane's checkpoint image on the host (ops/csrc/steplane_host.h namespace lane), no device: the
digest of small payloads against values worked out by hand and under every order of the chunks, the header
check's refusals (a short buffer, bad magic, a bad version, another kind, another array count or size, payload
bytes that do not match, another configuration by the field's name), every tracker's fingerprint and
``SlotRing::resume``. A stand-alone program walks them, built with AddressSanitizer + UBSan.
tests/test_tracker_checkpoint_gpu.py holds the image on the device."""

import os
import shutil
import subprocess

import pytest


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.timeout(300)
def test_lane_image_host_side_under_address_and_ub_sanitizers(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "llm_slo_ebpf_toolkit_amd", "ops", "csrc")
    exe = tmp_path / "steplane_image_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-Wall", "-Werror", f"-I{csrc}", os.path.join(root, "tests", "native", "steplane_image_check.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "steplane image ok" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
