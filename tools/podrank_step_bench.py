#!/usr/bin/env python3
"""Device time of one pod-breakdown step (ops/podrank.py), device events around ``step``.

The benchmark's span shape: 16,383 spans per window over 64 services and 256 pods, half of them
first-token records (observed: log-normal TTFTs, median 300 ms with a heavy tail) and half request
spans (SPAN_NO_SLI, skipped), K = 3 pods over a horizon of 3 windows. Prints the median, min and max of
the timed steps after the warm-up -- copy + kernels, kernels alone and the observe kernel alone -- as
one JSON line. ``--shape one-pair`` times the contention shape instead (every record observed, one
service, one pod), ``--shape wide`` one service with ``--pods`` pods (4,096 by default there);
``--no-lds`` runs the observe kernel without its per-workgroup LDS table, the measurement's other side.

    python tools/podrank_step_bench.py [--steps 200] [--warmup 30] [--spans 16383] [--groups 64] [--pods 256]
        [--k 3] [--windows 3] [--pairs 4096] [--shape bench|one-pair|wide] [--no-lds]
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
    ap.add_argument("--pods", type=int, default=0, help="pods (0: 256, or 4096 with --shape wide)")
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--shape", choices=("bench", "one-pair", "wide"), default="bench")
    ap.add_argument("--no-lds", action="store_true")
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args(argv)

    from llm_slo_ebpf_toolkit_amd.collector import records as R
    from llm_slo_ebpf_toolkit_amd.ops.podrank import PodRankTracker
    from llm_slo_ebpf_toolkit_amd.pipeline.podrank import stats_dict

    rng = np.random.default_rng(a.seed)
    pods = a.pods or (4096 if a.shape == "wide" else 256)

    def window() -> np.ndarray:
        s = np.zeros(a.spans, R.SPAN)
        s["trace_h"] = rng.integers(1, 1 << 63, a.spans, dtype=np.uint64)
        s["ttft_ms"] = rng.lognormal(np.log(300.0), 1.5, a.spans).astype(np.float32)
        if a.shape == "bench":
            s["pod_id"] = 1 + rng.integers(0, pods, a.spans)
            s["group_id"] = (s["pod_id"] - 1) % a.groups  # a pod serves one service: pods / groups replicas each
            s["flags"] = np.where(np.arange(a.spans) % 2 == 0, R.SPAN_FIRST_TOKEN, R.SPAN_NO_SLI)
            return np.ascontiguousarray(s[rng.permutation(a.spans)])
        s["flags"] = R.SPAN_FIRST_TOKEN
        s["pod_id"] = 9 if a.shape == "one-pair" else 1 + rng.integers(0, pods, a.spans)
        return s

    pool = [window() for _ in range(8)]
    t = PodRankTracker(k=a.k, windows=a.windows, pair_cap=a.pairs, span_cap=max(a.spans, 1), group_cap=a.groups,
                       n_buffers=3, lds=not a.no_lds)
    both, kern, obs, seen = [], [], [], []
    for w in range(a.warmup + a.steps):
        i = t.step_records(pool[w % len(pool)], a.groups)
        r = t.results(i, a.groups)
        if w >= a.warmup:
            ms = t.step_ms(i)
            both.append(ms[0])
            kern.append(ms[1])
            obs.append(t.observe_ms(i))
            seen.append(stats_dict(r["stats"])["observed"])
    st = stats_dict(r["stats"])
    pods_seen, pods_breaching = int(r["rec_pods"].sum()), int(r["rec_pods_b"].sum())
    t.close()
    us = lambda v: round(1e3 * float(v), 2)  # noqa: E731
    out = {"metric": "podrank_step_us", "shape": a.shape, "lds": not a.no_lds, "steps": a.steps, "warmup": a.warmup,
           "groups": a.groups, "pods": pods, "k": a.k, "windows": a.windows, "pair_cap": a.pairs,
           "spans_per_window": a.spans, "observed_per_window": int(np.median(seen)),
           "recent_pairs": pods_seen, "recent_pairs_breaching": pods_breaching, "pair_overflow": st["pair_overflow"]}
    for name, v in (("step", both), ("kernels", kern), ("observe", obs)):
        out.update({f"{name}_us_median": us(np.median(v)), f"{name}_us_min": us(np.min(v)),
                    f"{name}_us_max": us(np.max(v))})
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
