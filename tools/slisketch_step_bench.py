#!/usr/bin/env python3
"""Device time of one TTFT sketch step (ops/slisketch.py), device events around ``step``.

The benchmark's span shape: 16,383 spans per window over 64 services, half of them first-token
records (observed: log-normal TTFTs, median 300 ms with a heavy tail) and half request spans
(SPAN_NO_SLI, skipped), a rolling horizon of 300 windows. Prints the median, min and max of the
timed steps after the warm-up, copy + kernels and kernels alone, as one JSON line.

    python tools/slisketch_step_bench.py [--steps 200] [--warmup 30] [--spans 16383] [--groups 64] [--windows 300]
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
    ap.add_argument("--windows", type=int, default=300)
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args(argv)

    from llm_slo_ebpf_toolkit_amd.collector import records as R
    from llm_slo_ebpf_toolkit_amd.ops.slisketch import SliSketch
    from llm_slo_ebpf_toolkit_amd.pipeline.slisketch import stats_dict

    rng = np.random.default_rng(a.seed)

    def window() -> np.ndarray:
        s = np.zeros(a.spans, R.SPAN)
        s["group_id"] = rng.integers(0, a.groups, a.spans)
        s["ttft_ms"] = rng.lognormal(np.log(300.0), 1.5, a.spans).astype(np.float32)
        s["flags"] = np.where(np.arange(a.spans) % 2 == 0, R.SPAN_FIRST_TOKEN, R.SPAN_NO_SLI)
        return np.ascontiguousarray(s[rng.permutation(a.spans)])

    pool = [window() for _ in range(8)]
    t = SliSketch(span_cap=max(a.spans, 1), group_cap=a.groups, windows=a.windows, n_buffers=3)
    both, kern, seen = [], [], []
    for w in range(a.warmup + a.steps):
        i = t.step_records(pool[w % len(pool)], a.groups)
        r = t.results(i, a.groups)
        if w >= a.warmup:
            ms = t.step_ms(i)
            both.append(ms[0])
            kern.append(ms[1])
            seen.append(stats_dict(r["stats"])["observed"])
    n_roll = int(r["n_roll"].astype(np.int64).sum())
    t.close()
    us = lambda v: round(1e3 * float(v), 2)  # noqa: E731
    print(json.dumps({"metric": "slisketch_step_us", "steps": a.steps, "warmup": a.warmup, "groups": a.groups,
                      "windows": a.windows, "spans_per_window": a.spans, "observed_per_window": int(np.median(seen)),
                      "rolling_records": n_roll,
                      "step_us_median": us(np.median(both)), "step_us_min": us(np.min(both)),
                      "step_us_max": us(np.max(both)), "kernels_us_median": us(np.median(kern)),
                      "kernels_us_min": us(np.min(kern)), "kernels_us_max": us(np.max(kern))}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
