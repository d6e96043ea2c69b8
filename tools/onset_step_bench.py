#!/usr/bin/env python3
"""Device time of one breach-onset step (ops/onset.py), device events around ``step``.

The benchmark's span shape: 16,383 spans per window over 64 services, half of them first-token records
(observed: log-normal TTFTs, median 300 ms with a heavy tail, start times spread over the window's 16
bins) and half request spans (SPAN_NO_SLI, skipped), a ring of 1,024 bins, cuts one window apart.
Prints the median, min and max of the timed steps after the warm-up -- copy + kernels, kernels alone
and the observe kernel alone -- as one JSON line. ``--shape one-bin`` times the contention shape instead
(every record observed, one service, one bin), ``--shape spread`` one service over its window's 16 bins;
``--no-lds`` runs the observe kernel without its per-workgroup LDS table, the measurement's other side.

    python tools/onset_step_bench.py [--steps 200] [--warmup 30] [--spans 16383] [--groups 64] [--bins 1024]
        [--window-bins 16] [--shape bench|one-bin|spread] [--no-lds]
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
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--window-bins", type=int, default=16)
    ap.add_argument("--bin-ms", type=float, default=125.0)
    ap.add_argument("--shape", choices=("bench", "one-bin", "spread"), default="bench")
    ap.add_argument("--no-lds", action="store_true")
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args(argv)

    from llm_slo_ebpf_toolkit_amd.collector import records as R
    from llm_slo_ebpf_toolkit_amd.ops.onset import OnsetTracker
    from llm_slo_ebpf_toolkit_amd.pipeline.onset import stats_dict

    rng = np.random.default_rng(a.seed)
    bin_ns = int(round(a.bin_ms * 1e6))
    q_start = 1_700_000_000_000_000_000 // bin_ns

    def window():
        """(records, bins back from the cut's bin per record): the start times are set per step."""
        s = np.zeros(a.spans, R.SPAN)
        s["trace_h"] = rng.integers(1, 1 << 63, a.spans, dtype=np.uint64)
        s["ttft_ms"] = rng.lognormal(np.log(300.0), 1.5, a.spans).astype(np.float32)
        back = rng.integers(0, a.window_bins, a.spans)
        if a.shape == "bench":
            s["group_id"] = rng.integers(0, a.groups, a.spans)
            s["flags"] = np.where(np.arange(a.spans) % 2 == 0, R.SPAN_FIRST_TOKEN, R.SPAN_NO_SLI)
            p = rng.permutation(a.spans)
            return np.ascontiguousarray(s[p]), back[p]
        s["flags"] = R.SPAN_FIRST_TOKEN
        return s, (np.zeros(a.spans, np.int64) if a.shape == "one-bin" else back)

    pool = [window() for _ in range(8)]
    t = OnsetTracker(bins=a.bins, bin_ns=bin_ns, span_cap=max(a.spans, 1), group_cap=a.groups, n_buffers=3,
                     lds=not a.no_lds)
    both, kern, obs, seen = [], [], [], []
    for w in range(a.warmup + a.steps):
        q_hi = q_start + a.window_bins * (w + 1)
        recs, back = pool[w % len(pool)]
        recs["ts_ns"] = (q_hi - back) * bin_ns + 1
        i = t.step_records(recs, q_hi * bin_ns + bin_ns // 2, a.groups)
        r = t.results(i, a.groups)
        if w >= a.warmup:
            ms = t.step_ms(i)
            both.append(ms[0])
            kern.append(ms[1])
            obs.append(t.observe_ms(i))
            seen.append(stats_dict(r["stats"])["observed"])
    rows = r["rows"]
    t.close()
    us = lambda v: round(1e3 * float(v), 2)  # noqa: E731
    out = {"metric": "onset_step_us", "shape": a.shape, "lds": not a.no_lds, "steps": a.steps, "warmup": a.warmup,
           "groups": a.groups, "bins": a.bins, "window_bins": a.window_bins, "bin_ms": a.bin_ms,
           "spans_per_window": a.spans, "observed_per_window": int(np.median(seen)),
           "ring_requests": int(rows["n_ring"].sum()), "ring_breaches": int(rows["b_ring"].sum()),
           "services_in_alarm": int((rows["state"] == 2).sum())}
    for name, v in (("step", both), ("kernels", kern), ("observe", obs)):
        out.update({f"{name}_us_median": us(np.median(v)), f"{name}_us_min": us(np.min(v)),
                    f"{name}_us_max": us(np.max(v))})
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
