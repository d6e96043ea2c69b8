#!/usr/bin/env python3
"""Device time of one request-exemplar step (ops/exemplars.py), device events around ``step``.

The benchmark's span shape: 16,383 spans per window over 64 services, half of them first-token
records (observed: log-normal TTFTs, median 300 ms with a heavy tail) and half request spans
(SPAN_NO_SLI, skipped), K = 3 exemplars over a horizon of 3 windows. Prints the median, min and max
of the timed steps after the warm-up -- copy + kernels, kernels alone and the select kernel alone --
as one JSON line. ``--shape one-group`` times the contention shape instead (every record observed,
one service, all at 437.5 ms, or ``ascending`` / ``descending`` distinct values); ``--no-lds`` runs
the select kernel without its LDS privatisation, the measurement's other side.

    python tools/exemplars_step_bench.py [--steps 200] [--warmup 30] [--spans 16383] [--groups 64] [--k 3]
        [--windows 3] [--shape bench|one-group|ascending|descending] [--no-lds]
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
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--shape", choices=("bench", "one-group", "ascending", "descending"), default="bench")
    ap.add_argument("--no-lds", action="store_true")
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args(argv)

    from llm_slo_ebpf_toolkit_amd.collector import records as R
    from llm_slo_ebpf_toolkit_amd.ops.exemplars import ExemplarTracker
    from llm_slo_ebpf_toolkit_amd.pipeline.exemplars import stats_dict

    rng = np.random.default_rng(a.seed)

    def window() -> np.ndarray:
        s = np.zeros(a.spans, R.SPAN)
        s["trace_h"] = rng.integers(1, 1 << 63, a.spans, dtype=np.uint64)
        s["span_h"] = rng.integers(1, 1 << 63, a.spans, dtype=np.uint64)
        if a.shape == "bench":
            s["group_id"] = rng.integers(0, a.groups, a.spans)
            s["ttft_ms"] = rng.lognormal(np.log(300.0), 1.5, a.spans).astype(np.float32)
            s["flags"] = np.where(np.arange(a.spans) % 2 == 0, R.SPAN_FIRST_TOKEN, R.SPAN_NO_SLI)
            return np.ascontiguousarray(s[rng.permutation(a.spans)])
        s["flags"] = R.SPAN_FIRST_TOKEN
        ramp = 100.0 + 0.25 * np.arange(a.spans, dtype=np.float32)
        s["ttft_ms"] = {"one-group": np.full(a.spans, 437.5, np.float32), "ascending": ramp,
                        "descending": ramp[::-1]}[a.shape]
        return s

    pool = [window() for _ in range(8)]
    t = ExemplarTracker(k=a.k, windows=a.windows, span_cap=max(a.spans, 1), group_cap=a.groups, n_buffers=3,
                        lds=not a.no_lds)
    both, kern, sel, seen = [], [], [], []
    for w in range(a.warmup + a.steps):
        i = t.step_records(pool[w % len(pool)], a.groups)
        r = t.results(i, a.groups)
        if w >= a.warmup:
            ms = t.step_ms(i)
            both.append(ms[0])
            kern.append(ms[1])
            sel.append(t.select_ms(i))
            seen.append(stats_dict(r["stats"])["observed"])
    worst = float(r["recent"]["ttft_ms"][r["k_recent"] > 0, 0].max()) if (r["k_recent"] > 0).any() else None
    t.close()
    us = lambda v: round(1e3 * float(v), 2)  # noqa: E731
    out = {"metric": "exemplars_step_us", "shape": a.shape, "lds": not a.no_lds, "steps": a.steps, "warmup": a.warmup,
           "groups": a.groups, "k": a.k, "windows": a.windows, "spans_per_window": a.spans,
           "observed_per_window": int(np.median(seen)), "worst_recent_ttft_ms": worst}
    for name, v in (("step", both), ("kernels", kern), ("select", sel)):
        out.update({f"{name}_us_median": us(np.median(v)), f"{name}_us_min": us(np.min(v)),
                    f"{name}_us_max": us(np.max(v))})
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
