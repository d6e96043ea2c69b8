"""TTFT phase split on the host: the rules of the retrieval SLI tracker.

The first question about a TTFT breach of a RAG service is whether the retrieval or the model was slow. A
trace's first record carries its TTFT and, where the application reports a breakdown, the sum of its
retrieval times (``SPAN.retr_ms``, collector/otlp.py). Per step (one window, the span ranges the engine
gets) this tracker yields, per service (incident group), for the window and for the last ``windows`` steps
(the rolling horizon): a histogram of the retrieval time and one of the **model time** (TTFT minus
retrieval) with their p50 / p90 / p95 / p99 buckets, the exact sums of retrieval time and of TTFT, six
counters of requests by TTFT-breach phase, the SLI-counting records seen (the coverage's denominator), and
a verdict over the horizon with the steps it has held.

**Which records count**, checked in this order: a record with SPAN_START is skipped silently;
``group_id >= n_groups`` counts in ``out_of_group``; ``ttft_ms >= 0`` failing in float32 (NaN, negatives)
in ``invalid``; a record without SPAN_NO_SLI adds 1 to the service's ``sli``; ``0 < retr_ms < 1e7``
failing in float32 (NaN included) counts in ``no_breakdown``; anything else is **observed**. An observed
record that carries SPAN_NO_SLI also counts in ``extra`` (its breakdown reached the receiver after the
trace's first record left), so coverage may pass 1 by these. SPAN_LATE and SPAN_FIRST_TOKEN do not matter.

**Units**: 10 us. ``r = min(rint(float64(retr_ms) * 100), 2^24 - 1)``, ``t`` the same of ``ttft_ms``,
``slo_u`` the same of the float32 ``slo_ms`` (``rint`` rounds half to even and is monotone, so ``ttft_ms <=
slo_ms`` implies ``t <= slo_u``); ``budget_u`` the same of ``retrieval_budget_ms``, clamped to ``[1, 2^24 -
1]``. Model time ``m = t - r`` where ``t > r``, else 0; ``r > t`` counts in ``exceeds_ttft`` and is
observed all the same. Everything after these conversions is integer.

**Cells**: ``tb = ttft_ms > slo_ms`` (float32), ``rb = r > budget_u``. Not ``tb``: ``ok`` (0) or
``ok_slow_retrieval`` (1) by ``rb``. ``tb`` and ``m > slo_u`` (a breach even with free retrieval):
``model`` (2) or ``model_slow_retrieval`` (3) by ``rb``. ``tb``, ``m <= slo_u`` and ``rb``: ``retrieval``
(4). ``tb`` otherwise: ``combined`` (5), each phase within its own limit and the sum over.

**Buckets**: the decode SLI's rule (pipeline/decodesli.py ``bucket_of``) on ``r`` and on ``m``, K = 336
each; 0 is bucket 0. Quantiles are nearest-rank over the buckets (pipeline/slisketch.py ``rank_buckets``).

**Verdict** over the rolling row, with ``n`` the sum of the six cells, ``B`` cells 2..5, ``M`` cells 2 + 3,
``R`` cell 4: ``unknown`` (0) when ``n < min_requests`` or ``n * 10^6 < coverage_ppm * sli``; ``ok`` (1)
when ``B * 10^6 <= budget_ppm * n``; ``retrieval_bound`` (2) when ``R * 10^6 >= dominance_ppm * B``;
``model_bound`` (3) when ``M * 10^6 >= dominance_ppm * B``; else ``mixed`` (4). ``age`` counts the
consecutive steps with the same verdict, this one included, and saturates at 2^32 - 1.

``RetrievalSliOracle`` is the rules in numpy: the reference the device tracker (ops/csrc/retrsli.hip,
ops/retrsli.py) is tested against for equality, and what ``engine="cpu"`` uses.
"""

from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from ..collector import records
from .decodesli import K, bucket_of, lower, representative  # noqa: F401 - the histograms' rule
from .errsli import budget_ppm  # noqa: F401 - the error budget of an SLO target, in millionths
from .slisketch import EMPTY, PERMILLE, QUANTILE_NAMES, rank_buckets  # noqa: F401 - the sketch's rank rule
from .trackerstate import OracleCheckpoint

UNITS_PER_MS = 100.0
UNIT_MAX = (1 << 24) - 1
RETR_MAX_MS = np.float32(1e7)
N_CELLS = 6
CELL_STRIDE = 8
CELLS = ("ok", "ok_slow_retrieval", "model", "model_slow_retrieval", "retrieval", "combined")
STATES = ("unknown", "ok", "retrieval_bound", "model_bound", "mixed")
PPM = 10 ** 6
# per-step statistics, in the device's order (ops/csrc/retrsli_host.h Stat)
STATS = ("observed", "out_of_group", "invalid", "no_breakdown", "extra", "exceeds_ttft")
N_STATS = 8
EVENT_STATS = ("out_of_group", "invalid", "no_breakdown", "extra", "exceeds_ttft")
RESULT_FIELDS = ("cells", "cells_roll", "sum_r", "sum_t", "sum_r_roll", "sum_t_roll", "sli", "sli_roll", "q_r_win",
                 "q_r_roll", "q_m_win", "q_m_roll", "state", "age", "stats")
# what WindowPipeline.results() gains with the tracker on
RESULT_KEYS = ("retr_cells", "retr_cells_roll", "retr_sum_ms", "retr_ttft_sum_ms", "retr_sum_ms_roll",
               "retr_ttft_sum_ms_roll", "retr_sli", "retr_sli_roll", "retr_q", "retr_q_roll", "retr_model_q",
               "retr_model_q_roll", "retr_state", "retr_age")
STATE_WORDS = 2 * K + CELL_STRIDE + 4


def stats_dict(stats: np.ndarray) -> Dict[str, int]:
    return {name: int(stats[i]) for i, name in enumerate(STATS)}


def units_of_ms(ms) -> np.ndarray:
    """Times in units of 10 us (int64, ``ms``'s shape): ``min(rint(float64(ms) * 100), 2^24 - 1)``; a
    negative or NaN value gives 0."""
    with np.errstate(invalid="ignore"):
        x = np.rint(np.asarray(ms).astype(np.float64) * UNITS_PER_MS)
        x = np.where(x >= 0.0, np.minimum(x, float(UNIT_MAX)), 0.0)
    return x.astype(np.int64)


def budget_units(budget_ms: float) -> int:
    x = float(np.rint(float(budget_ms) * UNITS_PER_MS))
    return int(min(UNIT_MAX, x)) if x >= 1.0 else 1


def cell_of(tb, r, m, slo_u: int, budget_u: int) -> np.ndarray:
    """The breach-phase cell (int64) of observed records: ``tb`` their TTFT breach, ``r`` / ``m`` in units."""
    tb, rb = np.asarray(tb, dtype=bool), np.asarray(r) > budget_u
    mb = np.asarray(m) > slo_u
    return np.where(~tb, rb.astype(np.int64), np.where(mb, 2 + rb.astype(np.int64), np.where(rb, 4, 5)))


def state_of(cells: Sequence[int], sli: int, min_requests: int, coverage_ppm: int, budget_ppm: int,
             dominance_ppm: int) -> int:
    """The verdict of one service's rolling cells and SLI count, on Python integers."""
    c = [int(x) for x in cells]
    n = sum(c)
    if n < int(min_requests) or n * PPM < int(coverage_ppm) * int(sli):
        return 0
    M, R = c[2] + c[3], c[4]
    B = M + R + c[5]
    if B * PPM <= int(budget_ppm) * n:
        return 1
    if R * PPM >= int(dominance_ppm) * B:
        return 2
    if M * PPM >= int(dominance_ppm) * B:
        return 3
    return 4


def age_of(state: int, prev_state: int, prev_age: int) -> int:
    return 1 if state != prev_state else min(0xFFFFFFFF, prev_age + 1)


def _to_ms(q: np.ndarray) -> np.ndarray:
    q = np.asarray(q).astype(np.int64)
    return np.where(q == EMPTY, np.nan, representative()[np.minimum(q, K - 1)] / UNITS_PER_MS)


def result_keys(result: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """A step's results under the names WindowPipeline.results() carries (RESULT_KEYS): sums and quantiles
    in ms, a quantile NaN for an empty service."""
    def ms(name):
        return np.asarray(result[name]).astype(np.float64) / UNITS_PER_MS

    return {"retr_cells": np.asarray(result["cells"]), "retr_cells_roll": np.asarray(result["cells_roll"]),
            "retr_sum_ms": ms("sum_r"), "retr_ttft_sum_ms": ms("sum_t"), "retr_sum_ms_roll": ms("sum_r_roll"),
            "retr_ttft_sum_ms_roll": ms("sum_t_roll"), "retr_sli": np.asarray(result["sli"]),
            "retr_sli_roll": np.asarray(result["sli_roll"]), "retr_q": _to_ms(result["q_r_win"]),
            "retr_q_roll": _to_ms(result["q_r_roll"]), "retr_model_q": _to_ms(result["q_m_win"]),
            "retr_model_q_roll": _to_ms(result["q_m_roll"]), "retr_state": np.asarray(result["state"]),
            "retr_age": np.asarray(result["age"])}


def empty_result(n_groups: int) -> Dict[str, np.ndarray]:
    G = int(n_groups)
    out = {}
    for name in RESULT_FIELDS:
        if name.startswith("cells"):
            out[name] = np.zeros((G, N_CELLS), np.uint32)
        elif name.startswith("sum_"):
            out[name] = np.zeros(G, np.uint64)
        elif name.startswith("q_"):
            out[name] = np.full((G, len(PERMILLE)), EMPTY, np.uint32)
        elif name == "stats":
            out[name] = np.zeros(N_STATS, np.uint32)
        else:
            out[name] = np.zeros(G, np.uint32)
    return out


def summary(cells, sum_r_ms, sum_t_ms, sli, q_r_ms, q_m_ms) -> Dict[str, object]:
    """One service's cells, sums (ms), SLI count and quantiles (ms) as the decision log carries them; ``None``
    where a denominator is none. ``coverage`` = observed / SLI records; ``share`` = retrieval time / TTFT,
    a ratio of the two exact sums; ``model_ms.mean`` = mean TTFT minus mean retrieval (not below 0)."""
    c = [int(x) for x in cells]
    n, sli = sum(c), int(sli)
    names = ("p50", "p90", "p95", "p99")

    def quantiles(q):
        return {name: (None if n == 0 or not np.isfinite(q[j]) else round(float(q[j]), 4)) for j, name in enumerate(names)}

    rq, mq = quantiles(q_r_ms), quantiles(q_m_ms)
    rq["mean"] = None if n == 0 else round(float(sum_r_ms) / n, 4)
    mq["mean"] = None if n == 0 else round(max(0.0, float(sum_t_ms) - float(sum_r_ms)) / n, 4)
    return {"requests": n, "coverage": None if sli == 0 else round(n / sli, 6),
            "share": None if not float(sum_t_ms) > 0 else round(float(sum_r_ms) / float(sum_t_ms), 6),
            "phases": dict(zip(CELLS, c)), "retrieval_ms": rq, "model_ms": mq}


def entry(res: Dict[str, np.ndarray], g: int) -> Dict[str, object]:
    """Group ``g`` of a window's ``retr_*`` results (RESULT_KEYS) as the decision log carries it: the
    horizon's verdict and the steps it has held, the window's summary, and the horizon's."""
    return {"state": STATES[int(res["retr_state"][g])], "age_windows": int(res["retr_age"][g]),
            **summary(res["retr_cells"][g], res["retr_sum_ms"][g], res["retr_ttft_sum_ms"][g], res["retr_sli"][g],
                      res["retr_q"][g], res["retr_model_q"][g]),
            "horizon": summary(res["retr_cells_roll"][g], res["retr_sum_ms_roll"][g], res["retr_ttft_sum_ms_roll"][g],
                               res["retr_sli_roll"][g], res["retr_q_roll"][g], res["retr_model_q_roll"][g])}


# ---- layout and checks (ops/csrc/retrsli_host.h) --------------------------------------------------
def layout(group_cap: int) -> Dict[str, int]:
    """Word offsets of the result block's arrays (every array on 16 bytes) and its ``words``."""
    g = int(group_cap)
    pair, one = (2 * g + 3) & ~3, (g + 3) & ~3
    off, at = {}, 0
    for name in RESULT_FIELDS:
        off[name] = at
        at += (CELL_STRIDE * g if name.startswith("cells") else pair if name.startswith("sum_") else 4 * g
               if name.startswith("q_") else N_STATS if name == "stats" else one)
    off["words"] = at
    return off


def device_bytes(span_cap: int, group_cap: int, windows: int) -> int:
    return (int(span_cap) * 64 + (int(windows) + 2) * int(group_cap) * STATE_WORDS * 4 + int(group_cap) * 2 * 4
            + layout(group_cap)["words"] * 4)


def check_config(span_cap: int, group_cap: int, windows: int, n_buffers: int, slo_ms: float, retrieval_budget_ms: float,
                 budget_ppm: int, coverage_ppm: int, dominance_ppm: int, min_requests: int) -> None:
    """The configuration checks of ops/csrc/retrsli_host.h validate()."""
    if not 1 <= windows <= 4096:
        raise ValueError("retrieval sli: windows must be in [1, 4096]")
    if not 1 <= group_cap <= 65536:
        raise ValueError("retrieval sli: group_cap must be in [1, 65536]")
    if span_cap < 1:
        raise ValueError("retrieval sli: span_cap must be >= 1")
    if span_cap * windows >= 1 << 32:
        raise ValueError("retrieval sli: span_cap * windows must stay below 2^32 (a rolling counter would wrap)")
    if not 1 <= n_buffers <= 64:
        raise ValueError("retrieval sli: n_buffers out of range")
    if not (np.isfinite(slo_ms) and slo_ms >= 0):
        raise ValueError("retrieval sli: slo_ms must be finite and >= 0")
    if not (np.isfinite(retrieval_budget_ms) and retrieval_budget_ms > 0):
        raise ValueError("retrieval sli: retrieval_budget_ms must be finite and > 0")
    if not 1 <= budget_ppm <= 999999:
        raise ValueError("retrieval sli: budget_ppm must be in [1, 999999]")
    if not 0 <= coverage_ppm <= 1000000:
        raise ValueError("retrieval sli: coverage_ppm must be in [0, 1000000]")
    if not 500000 < dominance_ppm <= 1000000:
        raise ValueError("retrieval sli: dominance_ppm must be in (500000, 1000000]")
    if not 1 <= min_requests <= (1 << 31) - 1:
        raise ValueError("retrieval sli: min_requests must be in [1, 2^31 - 1]")
    if device_bytes(span_cap, group_cap, windows) > 1 << 31:
        raise ValueError("retrieval sli: the horizon needs more than 2 GiB")
    if layout(group_cap)["words"] * 4 > 1 << 31:
        raise ValueError("retrieval sli: a result block needs more than 2 GiB")


def block_of(result: Dict[str, np.ndarray], group_cap: int) -> np.ndarray:
    """A step's results over all ``group_cap`` rows as the device's result block (uint32 words)."""
    off = layout(group_cap)
    out = np.zeros(off["words"], np.uint32)
    for name in RESULT_FIELDS:
        a = np.ascontiguousarray(result[name])
        if name.startswith("cells"):
            pad = np.zeros((len(a), CELL_STRIDE), np.uint32)
            pad[:, :N_CELLS] = a
            a = pad
        w = a.view(np.uint32).reshape(-1)
        out[off[name]:off[name] + len(w)] = w
    return out


def _gather(ranges) -> np.ndarray:
    from .cpu import _gather as g

    b = g(ranges)
    return b.view(records.SPAN) if len(b) else np.zeros(0, records.SPAN)


class RetrievalSliOracle(OracleCheckpoint):
    """The tracker's rules in numpy (see the module docstring), with the device handle's interface."""

    # checkpoint (pipeline/trackerstate.py): the fields ops/csrc/retrsli_host.h fingerprint() covers, and what is
    # kept between steps
    KIND = "retrieval sli"
    FINGERPRINT = ("group_cap", "windows", "slo_ms", "retrieval_budget_ms", "th")
    STATE = ("roll_r", "roll_m", "cells_roll", "sli_roll", "sum_roll", "verdict", "age", "held", "n")

    def __init__(self, span_cap: int = 16384, group_cap: int = 64, windows: int = 150, n_buffers: int = 3,
                 slo_ms: float = 800.0, retrieval_budget_ms: float = 200.0, budget_ppm: int = 10000,
                 coverage_ppm: int = 500000, dominance_ppm: int = 667000, min_requests: int = 200, device: int = 0,
                 lds: bool = True):
        span_cap, group_cap, windows, n_buffers = int(span_cap), int(group_cap), int(windows), int(n_buffers)
        self.th = dict(min_requests=int(min_requests), coverage_ppm=int(coverage_ppm), budget_ppm=int(budget_ppm),
                       dominance_ppm=int(dominance_ppm))
        check_config(span_cap, group_cap, windows, n_buffers, float(slo_ms), float(retrieval_budget_ms), **self.th)
        self.span_cap, self.group_cap, self.windows, self.nb = span_cap, group_cap, windows, n_buffers
        self.slo_ms, self.retrieval_budget_ms = float(slo_ms), float(retrieval_budget_ms)
        self.slo_units = int(units_of_ms(np.float32(slo_ms)))
        self.budget_units = budget_units(retrieval_budget_ms)
        self.roll_r = np.zeros((group_cap, K), np.int64)
        self.roll_m = np.zeros((group_cap, K), np.int64)
        self.cells_roll = np.zeros((group_cap, N_CELLS), np.int64)
        self.sli_roll = np.zeros(group_cap, np.int64)
        self.sum_roll = np.zeros((group_cap, 2), np.uint64)
        self.verdict = np.zeros(group_cap, np.uint32)  # the published state of the step before
        self.age = np.zeros(group_cap, np.uint32)
        self.held: Dict[int, tuple] = {}  # step % windows -> that step's rows
        self.res: Dict[int, Tuple[int, dict]] = {}
        self.n = 0

    # ---- one window ---------------------------------------------------------------------------
    def step(self, span_ranges: Sequence[Tuple[int, int]], n_groups: int) -> int:
        """``span_ranges`` = [(host address, bytes)] of 64-byte SPAN records, as the engine gets them."""
        for a, nbytes in span_ranges:
            if int(nbytes) % 64:
                raise ValueError("retrieval sli step: a range is not whole 64-byte spans")
            if int(nbytes) and not int(a):
                raise ValueError("retrieval sli step: null range")
        return self.step_records(_gather(span_ranges), n_groups)

    def step_records(self, spans: np.ndarray, n_groups: int) -> int:
        G, C = int(n_groups), self.group_cap
        if not 0 <= G <= C:
            raise ValueError("retrieval sli step: n_groups out of range")
        if len(spans) > self.span_cap:
            raise ValueError("retrieval sli step: more spans than span_cap")
        # nothing has changed up to here
        fl = spans["flags"].astype(np.uint32)
        grp = spans["group_id"].astype(np.int64)
        v = np.ascontiguousarray(spans["ttft_ms"], dtype=np.float32)
        rm = np.ascontiguousarray(spans["retr_ms"], dtype=np.float32)
        live = (fl & np.uint32(records.SPAN_START)) == 0
        ingrp = live & (grp < G)
        nosli = (fl & np.uint32(records.SPAN_NO_SLI)) != 0
        with np.errstate(invalid="ignore"):
            valid = ingrp & (v >= np.float32(0.0))
            ok = valid & (rm > np.float32(0.0)) & (rm < RETR_MAX_MS)
        g = grp[ok]
        r, t = units_of_ms(rm[ok]), units_of_ms(v[ok])
        m = np.where(t > r, t - r, 0)
        hist_r, hist_m = np.zeros((C, K), np.int64), np.zeros((C, K), np.int64)
        np.add.at(hist_r, (g, bucket_of(r)), 1)
        np.add.at(hist_m, (g, bucket_of(m)), 1)
        cells = np.zeros((C, N_CELLS), np.int64)
        np.add.at(cells, (g, cell_of(v[ok] > np.float32(self.slo_ms), r, m, self.slo_units, self.budget_units)), 1)
        sums = np.zeros((C, 2), np.uint64)
        np.add.at(sums[:, 0], g, r.astype(np.uint64))
        np.add.at(sums[:, 1], g, t.astype(np.uint64))
        sli = np.zeros(C, np.int64)
        np.add.at(sli, grp[valid & ~nosli], 1)
        stats = np.zeros(N_STATS, np.uint32)
        stats[:len(STATS)] = [int(ok.sum()), int((live & ~ingrp).sum()), int((ingrp & ~valid).sum()), int((valid & ~ok).sum()),
                              int((ok & nosli).sum()), int((r > t).sum())]
        idx = self.n
        slot = idx % self.windows
        old = self.held.get(slot)
        if old is not None:
            self.roll_r -= old[0]
            self.roll_m -= old[1]
            self.cells_roll -= old[2]
            self.sum_roll -= old[3]
            self.sli_roll -= old[4]
        self.roll_r += hist_r
        self.roll_m += hist_m
        self.cells_roll += cells
        self.sum_roll += sums
        self.sli_roll += sli
        self.held[slot] = (hist_r, hist_m, cells, sums, sli)
        state = np.array([state_of(self.cells_roll[j], self.sli_roll[j], **self.th) for j in range(C)], np.uint32)
        self.age = np.array([age_of(int(state[j]), int(self.verdict[j]), int(self.age[j])) for j in range(C)], np.uint32)
        self.verdict = state
        res = {"cells": cells.astype(np.uint32), "cells_roll": self.cells_roll.astype(np.uint32),
               "sum_r": sums[:, 0].copy(), "sum_t": sums[:, 1].copy(), "sum_r_roll": self.sum_roll[:, 0].copy(),
               "sum_t_roll": self.sum_roll[:, 1].copy(), "sli": sli.astype(np.uint32), "sli_roll": self.sli_roll.astype(np.uint32),
               "q_r_win": rank_buckets(hist_r), "q_r_roll": rank_buckets(self.roll_r), "q_m_win": rank_buckets(hist_m),
               "q_m_roll": rank_buckets(self.roll_m), "state": state.copy(), "age": self.age.copy(), "stats": stats}
        self.res[idx % self.nb] = (idx, res)
        self.n += 1
        return idx

    # ---- results ------------------------------------------------------------------------------
    def query(self, i: int) -> bool:
        return True

    def _held(self, i: int) -> dict:
        held = self.res.get(int(i) % self.nb)
        if held is None or held[0] != int(i):
            raise IndexError(f"retrieval sli step {i} is not held (only the last {self.nb})")
        return held[1]

    def results(self, i: int, n_groups: int) -> Dict[str, np.ndarray]:
        res = self._held(i)
        G = int(n_groups)
        if not 0 <= G <= self.group_cap:
            raise ValueError("n_groups")
        return {k: (v.copy() if k == "stats" else v[:G].copy()) for k, v in res.items()}

    def block(self, i: int) -> np.ndarray:
        """Step ``i``'s results as the device's whole result block (uint32 words)."""
        return block_of(self._held(i), self.group_cap)

    def step_ms(self, i: int) -> Tuple[float, float]:
        return 0.0, 0.0

    def observe_ms(self, i: int) -> float:
        return 0.0

    def resident(self) -> Dict[str, np.ndarray]:
        """The rolling state: ``rows_r`` / ``rows_m`` [group_cap, K], ``cells`` [group_cap, 6], ``sli``
        [group_cap], ``sums`` [group_cap, 2] (retrieval, TTFT), ``state``, ``age`` and ``pos``, the horizon
        row the next step replaces."""
        return {"rows_r": self.roll_r.astype(np.uint32), "rows_m": self.roll_m.astype(np.uint32),
                "cells": self.cells_roll.astype(np.uint32), "sli": self.sli_roll.astype(np.uint32),
                "sums": self.sum_roll.copy(), "state": self.verdict.copy(), "age": self.age.copy(),
                "pos": self.n % self.windows}

    def sync(self) -> None:
        pass

    def close(self) -> None:
        pass
