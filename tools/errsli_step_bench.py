#!/usr/bin/env python3
"""Device time of one error SLI step (ops/errsli.py), device events around ``step``.

The benchmark's span shape: 16,383 spans per window over 64 services, half of them records that end a
request (observed; the class uniform over the eight) and half first-token records (skipped), the agent's
default pairs at one-second windows (3600:300:14.4 and 21600:1800:6, a horizon of 21,600 windows). Prints
the median, min and max of the timed steps after the warm-up -- copy + kernels, kernels alone and the
observe kernel alone -- as one JSON line. ``--shape one-key`` times the contention shape instead (every
record observed, one service, one class); ``--shape realistic`` every record observed, 64 services, each
mostly ``ok`` with 5 % in one failing class of its own; ``--no-lds`` runs the observe kernel without its
per-workgroup LDS table, the measurement's other side.

    python tools/errsli_step_bench.py [--steps 200] [--warmup 30] [--spans 16383] [--groups 64]
        [--pairs 3600:300:14.4,21600:1800:6] [--window-ms 1000] [--shape bench|one-key|realistic] [--no-lds]
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
    ap.add_argument("--pairs", default="3600:300:14.4,21600:1800:6")
    ap.add_argument("--window-ms", type=float, default=1000.0)
    ap.add_argument("--shape", choices=("bench", "one-key", "realistic"), default="bench")
    ap.add_argument("--no-lds", action="store_true")
    ap.add_argument("--seed", type=int, default=3)
    a = ap.parse_args(argv)

    from llm_slo_ebpf_toolkit_amd.collector import records as R
    from llm_slo_ebpf_toolkit_amd.ops.errsli import ErrorSliTracker
    from llm_slo_ebpf_toolkit_amd.pipeline import errsli as rules

    rng = np.random.default_rng(a.seed)
    pairs = rules.parse_pairs(a.pairs, a.window_ms)
    windows = max(p[0] for p in pairs)

    def window():
        s = np.zeros(a.spans, R.SPAN)
        s["trace_h"] = rng.integers(1, 1 << 63, a.spans, dtype=np.uint64)
        s["ttft_ms"] = rng.lognormal(np.log(300.0), 1.5, a.spans).astype(np.float32)
        if a.shape == "bench":
            s["group_id"] = rng.integers(0, a.groups, a.spans)
            final = np.arange(a.spans) % 2 == 0
            s["flags"] = np.where(final, R.pack_outcome(rng.integers(0, 8, a.spans)), R.SPAN_FIRST_TOKEN)
            return np.ascontiguousarray(s[rng.permutation(a.spans)])
        if a.shape == "one-key":
            s["flags"] = R.pack_outcome(np.full(a.spans, 6, np.int64))
            return s
        g = rng.integers(0, a.groups, a.spans)
        s["group_id"] = g
        s["flags"] = R.pack_outcome(np.where(rng.random(a.spans) < 0.05, 1 + g % 7, 0))
        return s

    pool = [window() for _ in range(8)]
    t = ErrorSliTracker(span_cap=max(a.spans, 1), group_cap=a.groups, windows=windows, n_buffers=3, pairs=pairs,
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
    t.close()
    us = lambda v: round(1e3 * float(v), 2)  # noqa: E731
    out = {"metric": "errsli_step_us", "shape": a.shape, "lds": not a.no_lds, "steps": a.steps, "warmup": a.warmup,
           "groups": a.groups, "windows": windows, "pairs": [list(p) for p in pairs], "spans_per_window": a.spans,
           "observed_per_window": int(np.median(seen)), "horizon_requests": int(r["counts_roll"].sum()),
           "firing_services": int((r["firing"] != 0).sum())}
    for name, v in (("step", both), ("kernels", kern), ("observe", obs)):
        out.update({f"{name}_us_median": us(np.median(v)), f"{name}_us_min": us(np.min(v)),
                    f"{name}_us_max": us(np.max(v))})
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
