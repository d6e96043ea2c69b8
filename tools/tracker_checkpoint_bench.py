"""Image bytes and snapshot times of the eleven device side trackers at their handles' default sizes
or, with ``--agent-flags``, at the sizes the agent's default flags give them
(docs/TRACKER_CHECKPOINT.md): per tracker a few steps of an empty window, then ``--repeat`` snapshots, each
timed three ways -- the gather and digest kernel on the device (events), the host time until ``snapshot()``
returns (the enqueue) and the wall time until the image is on the host -- and then the kernels time of an empty
step before a snapshot, of the step issued right after one (the transfer still running) and of the step after
that. One JSON line per tracker."""

from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HANDLES = {"openreq": "OpenRequestTable", "slisketch": "SliSketch", "exemplars": "ExemplarTracker",
           "podrank": "PodRankTracker", "onset": "OnsetTracker", "decodesli": "DecodeSliTracker", "drift": "DriftTracker",
           "errsli": "ErrorSliTracker", "loadsli": "LoadSliTracker", "satcurve": "SaturationTracker",
           "retrsli": "RetrievalSliTracker"}
CUTS = {"openreq": 2, "onset": 1, "loadsli": 1, "satcurve": 1}  # time arguments of a step


def agent_sizes() -> dict:
    """The sizes the agent gives its trackers at its default flags, where they are not the handles' defaults."""
    from llm_slo_ebpf_toolkit_amd.agent.daemon import Agent, AgentOptions

    a = Agent(AgentOptions())
    return {"slisketch": dict(windows=a.ttft_horizon()), "decodesli": dict(windows=a.decode_horizon()),
            "retrsli": dict(windows=a.retrieval_horizon()), "errsli": dict(windows=a.error_horizon(), pairs=a.error_pairs()),
            "drift": dict(zip(("recent", "gap", "baseline"), a.drift_windows())), "loadsli": a.load_params(),
            "satcurve": a.saturation_params()}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--agent-flags", action="store_true", help="the agent's default sizes, not the handles'")
    ap.add_argument("--trackers", default=",".join(HANDLES))
    a = ap.parse_args(argv)
    sizes = agent_sizes() if a.agent_flags else {}
    for name in [x for x in a.trackers.split(",") if x]:
        ops = importlib.import_module(f"llm_slo_ebpf_toolkit_amd.ops.{name}")
        t = getattr(ops, HANDLES[name])(**sizes.get(name, {}))
        try:
            for w in range(3):
                cut = (w + 1) * 10 ** 9
                t.step([], *((cut, cut - 10 ** 9 if w else 0)[:CUTS.get(name, 0)]), 1)
            t.sync()
            kernel_ms, enqueue_ms, host_ms = [], [], []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                ticket = t.snapshot()
                t1 = time.perf_counter()
                t.snapshot_image(ticket)
                t2 = time.perf_counter()
                kernel_ms.append(t.snapshot_kernel_ms())
                enqueue_ms.append((t1 - t0) * 1e3)
                host_ms.append((t2 - t0) * 1e3)

            def step(w):
                cut = (w + 1) * 10 ** 9
                return t.step([], *((cut, cut - 10 ** 9)[:CUTS.get(name, 0)]), 1)

            around = []
            for r in range(a.repeat):
                before = step(10 + 3 * r)
                t.sync()
                ticket = t.snapshot()
                after = step(11 + 3 * r)
                later = step(12 + 3 * r)
                t.snapshot_image(ticket)
                around.append([round(float(t.step_ms(i)[1]), 4) for i in (before, after, later)])
            med = statistics.median
            print(json.dumps({"tracker": name, "sizes": "agent" if a.agent_flags else "handle", "image_bytes": t.image_bytes(), "repeat": a.repeat,
                              "kernel_ms_median": round(med(kernel_ms[1:]), 4), "kernel_ms": [round(x, 4) for x in kernel_ms],
                              "enqueue_ms_median": round(med(enqueue_ms[1:]), 4),
                              "to_host_ms_median": round(med(host_ms[1:]), 3), "to_host_ms": [round(x, 3) for x in host_ms],
                              "step_kernels_ms_before_after_later_median": [round(med(x[k] for x in around[1:]), 4)
                                                                            for k in range(3)]}),
                  flush=True)
        finally:
            t.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
