#!/usr/bin/env python3
"""Device time of one TTFT drift step (ops/drift.py), device events around ``step``.

The benchmark's span shape: 16,383 spans per window over 64 services, every one observed (log-normal TTFTs,
median 300 ms with a heavy tail), the rings of a 1 s window (R = L = 10, B = 300). Prints the median, min and
max of the timed steps after the warm-up -- copy + kernels, kernels alone and the observe kernel alone -- as
one JSON line. ``--shape one-bucket`` times the contention shape instead (one service, one bucket);
``--shape realistic`` 64 services, each service's TTFTs in three adjacent buckets of its own; ``--no-lds``
runs the observe kernel without its per-workgroup LDS table, the measurement's other side.

    python tools/drift_step_bench.py [--steps 200] [--warmup 30] [--spans 16383] [--groups 64] [--window-ms 1000]
        [--shape bench|one-bucket|realistic] [--no-lds]
"""

from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--spans", type=int, default=16383)
    ap.add_argument("--groups", type=int, default=64)
    ap.add_argument("--window-ms", type=float, default=1000.0)
    ap.add_argument("--shape", choices=("bench", "one-bucket", "realistic"), default="bench")
    ap.add_argument("--no-lds", action="store_true")
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args(argv)

    from llm_slo_ebpf_toolkit_amd.collector import records as R
    from llm_slo_ebpf_toolkit_amd.ops.drift import DriftTracker
    from llm_slo_ebpf_toolkit_amd.pipeline import drift as rules
    from llm_slo_ebpf_toolkit_amd.pipeline import slisketch

    rng = np.random.default_rng(a.seed)
    edges = slisketch.bucket_edges()

    def window():
        s = np.zeros(a.spans, R.SPAN)
        s["trace_h"] = rng.integers(1, 1 << 63, a.spans, dtype=np.uint64)
        if a.shape == "bench":
            s["group_id"] = rng.integers(0, a.groups, a.spans)
            s["ttft_ms"] = rng.lognormal(np.log(300.0), 1.5, a.spans).astype(np.float32)
            return s
        if a.shape == "one-bucket":
            s["ttft_ms"] = np.float32(300.0)
            return s
        g = rng.integers(0, a.groups, a.spans)
        s["group_id"] = g
        first = 120 + (g % 32) * 3  # every service its own three adjacent buckets, 21 ms to 1.3 s
        s["ttft_ms"] = edges[first + rng.integers(0, 3, a.spans) - 1].astype(np.float32)
        return s

    pool = [window() for _ in range(8)]
    R_, L_, B_ = rules.defaults(a.window_ms)
    t = DriftTracker(span_cap=max(a.spans, 1), group_cap=a.groups, recent=R_, gap=L_, baseline=B_, n_buffers=3,
                     lds=not a.no_lds)
    both, kern, obs, seen = [], [], [], []
    for w in range(a.warmup + a.steps):
        i = t.step_records(pool[w % len(pool)], a.groups)
        r = t.results(i, a.groups)
        if w >= a.warmup:
            ms = t.step_ms(i)
            both.append(ms[0])
            kern.append(ms[1])
            obs.append(t.observe_ms(i))
            seen.append(rules.stats_dict(r["stats"])["observed"])
    buckets = (t.resident()["recent"] > 0).sum(axis=1)
    t.close()
    us = lambda v: round(1e3 * float(v), 2)  # noqa: E731
    out = {"metric": "drift_step_us", "shape": a.shape, "lds": not a.no_lds, "steps": a.steps, "warmup": a.warmup,
           "groups": a.groups, "recent": R_, "gap": L_, "baseline": B_, "spans_per_window": a.spans,
           "observed_per_window": int(np.median(seen)), "recent_records": int(r["n_recent"].sum()),
           "base_records": int(r["n_base"].sum()), "decided_services": int(((r["state"] & rules.WARMING) == 0).sum()),
           "buckets_per_service_max": int(buckets.max())}
    for name, v in (("step", both), ("kernels", kern), ("observe", obs)):
        out.update({f"{name}_us_median": us(np.median(v)), f"{name}_us_min": us(np.min(v)),
                    f"{name}_us_max": us(np.max(v))})
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
