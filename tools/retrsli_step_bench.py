#!/usr/bin/env python3
"""Device time of one TTFT phase split step (ops/retrsli.py), device events around ``step``.

The benchmark's span shape: 16,383 spans per window over 64 services, half of them first-token records that
carry a retrieval breakdown (observed: log-normal TTFTs, median 300 ms with a heavy tail; retrieval times
log-normal about 60 ms) and half final records with SPAN_NO_SLI and none (no_breakdown), a horizon of 150
windows. Prints the median, min and max of the timed steps after the warm-up -- copy + kernels, kernels alone
and the observe kernel alone -- as one JSON line. ``--shape one-key`` times the contention shape instead (every
record observed, one service, one retrieval bucket, one model bucket, one cell); ``--shape realistic`` every
record observed, 64 services, each service's retrieval and model times in three adjacent buckets of its own;
``--no-lds`` runs the observe kernel without its per-workgroup LDS table, the measurement's other side.

    python tools/retrsli_step_bench.py [--steps 200] [--warmup 30] [--spans 16383] [--groups 64] [--windows 150]
        [--shape bench|one-key|realistic] [--no-lds]
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
    ap.add_argument("--windows", type=int, default=150)
    ap.add_argument("--shape", choices=("bench", "one-key", "realistic"), default="bench")
    ap.add_argument("--no-lds", action="store_true")
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args(argv)

    from llm_slo_ebpf_toolkit_amd.collector import records as R
    from llm_slo_ebpf_toolkit_amd.ops.retrsli import RetrievalSliTracker
    from llm_slo_ebpf_toolkit_amd.pipeline import retrsli as rules

    rng = np.random.default_rng(a.seed)

    def window():
        s = np.zeros(a.spans, R.SPAN)
        s["trace_h"] = rng.integers(1, 1 << 63, a.spans, dtype=np.uint64)
        if a.shape == "bench":
            s["group_id"] = rng.integers(0, a.groups, a.spans)
            first = np.arange(a.spans) % 2 == 0
            retr = rng.lognormal(np.log(60.0), 0.8, a.spans)
            s["retr_ms"] = np.where(first, retr, 0.0).astype(np.float32)
            s["ttft_ms"] = (np.where(first, retr, 0.0) + rng.lognormal(np.log(300.0), 1.5, a.spans)).astype(np.float32)
            s["flags"] = np.where(first, R.SPAN_FIRST_TOKEN, R.SPAN_NO_SLI)
            return np.ascontiguousarray(s[rng.permutation(a.spans)])
        s["flags"] = R.SPAN_FIRST_TOKEN
        if a.shape == "one-key":
            s["retr_ms"], s["ttft_ms"] = 300.0, 900.0
            return s
        g = rng.integers(0, a.groups, a.spans)
        s["group_id"] = g
        # every service its own three adjacent buckets of each histogram: retrieval 10 ms to 640 ms, model time above it
        r_u = rules.lower(160 + (g % 32) * 3 + rng.integers(0, 3, a.spans))
        m_u = rules.lower(200 + (g % 16) * 3 + rng.integers(0, 3, a.spans))
        s["retr_ms"] = (r_u / 100.0).astype(np.float32)
        s["ttft_ms"] = ((r_u + m_u) / 100.0).astype(np.float32)
        return s

    pool = [window() for _ in range(8)]
    t = RetrievalSliTracker(span_cap=max(a.spans, 1), group_cap=a.groups, windows=a.windows, n_buffers=3, lds=not a.no_lds)
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
    res = t.resident()
    buckets_r, buckets_m = (res["rows_r"] > 0).sum(axis=1), (res["rows_m"] > 0).sum(axis=1)
    t.close()
    us = lambda v: round(1e3 * float(v), 2)  # noqa: E731
    out = {"metric": "retrsli_step_us", "shape": a.shape, "lds": not a.no_lds, "lds_slots": t.lds_slots, "steps": a.steps,
           "warmup": a.warmup, "groups": a.groups, "windows": a.windows, "spans_per_window": a.spans,
           "observed_per_window": int(np.median(seen)), "horizon_requests": int(r["cells_roll"].sum()),
           "horizon_sli": int(r["sli_roll"].sum()), "states": np.bincount(r["state"], minlength=5).tolist(),
           "retrieval_buckets_per_service_max": int(buckets_r.max()), "model_buckets_per_service_max": int(buckets_m.max())}
    for name, v in (("step", both), ("kernels", kern), ("observe", obs)):
        out.update({f"{name}_us_median": us(np.median(v)), f"{name}_us_min": us(np.min(v)),
                    f"{name}_us_max": us(np.max(v))})
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
