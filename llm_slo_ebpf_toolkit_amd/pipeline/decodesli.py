"""Decode-phase SLI on the host: the rules of the decode SLI tracker.

Every other SLI is a view of TTFT. A request has a second SLO that its user feels as much: the rate at
which the rest of the tokens arrive, time per output token (TPOT). Per step (one window, the span
ranges the engine gets) this tracker yields, per service (incident group), for the window and for the
last ``windows`` steps (the rolling horizon): a TPOT histogram and its p50 / p90 / p95 / p99 buckets,
the exact TPOT sum in microseconds, and the 2x2 table of requests by (TTFT breach, TPOT breach). Cell 0,
neither breached, over the requests is the service's **goodput**; the off-diagonal cells tell a
prefill problem (TTFT only) from a decode problem (TPOT only).

**The value**: a 64-byte SPAN carries its TPOT as integer microseconds in bits 8-31 of ``flags``
(``u = flags >> 8``, collector/records.py ``span_tpot_us``); 0 = no decode SLI, else 1 .. 2^24 - 1.

**Which records count**, checked in this order: a record with SPAN_START or SPAN_FIRST_TOKEN is
skipped silently; ``u == 0`` is counted in ``no_decode``; ``group_id >= n_groups`` in ``out_of_group``;
``ttft_ms >= 0`` failing in float32 (NaN, negatives) in ``invalid``; anything else is observed.
SPAN_NO_SLI and SPAN_LATE do not matter: this set is the requests that **finished** in the window,
whether or not a first-token record counted their TTFT earlier. Its ``n`` is therefore not the
window's ``sli`` count (which counts first tokens, in the window they happened in).

**Cells**: ``tb = ttft_ms > slo_ms`` (float32 compare), ``db = u > tpot_slo_us`` with ``tpot_slo_us =
clamp(int(tpot_slo_ms * 1000 + 0.5), 1, 2^24 - 1)``; cell ``tb + 2 * db``.

**Bucket**, read off the integer (no float, no logarithm -- host and device cannot differ): ``u < 16``
is its own bucket; else ``e = floor(log2 u)`` and ``b = 16 * (e - 3) + ((u >> (e - 4)) & 15)``: 16
linear sub-buckets per octave, K = 336 buckets up to 2^24 - 1. ``lower(b) = b`` below 16, else
``(16 + b % 16) << (b // 16 - 1)``. A bucket stands for the midpoint of the integers it holds: exact
below 16, within v / 32 of every v above.

Quantiles are nearest-rank over the buckets as in the TTFT sketch (pipeline/slisketch.py
``rank_buckets``): the bucket's index, EMPTY for a service without a record.

The horizon is counted in steps: every step evicts the step ``windows`` before it, in every row of
``group_cap``, histogram, table and sum alike.

``DecodeSliOracle`` is the rules in numpy: the reference the device tracker (ops/csrc/decodesli.hip,
ops/decodesli.py) is tested against for equality, and what ``engine="cpu"`` uses.
"""

from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

from ..collector import records
from .trackerstate import OracleCheckpoint
from .slisketch import EMPTY, PERMILLE, QUANTILE_NAMES, rank_buckets  # noqa: F401 - the sketch's rank rule

K = 336
PER_LANE = 6                 # buckets a lane of the roll kernel's wave owns
N_CELLS = 4
CELLS = ("good", "ttft_only", "tpot_only", "both")   # cell = tb + 2 * db
TPOT_MAX = records.SPAN_TPOT_MAX
SKIP = records.SPAN_START | records.SPAN_FIRST_TOKEN
# per-step statistics, in the device's order (ops/csrc/decodesli_host.h Stat)
STATS = ("observed", "invalid", "out_of_group", "no_decode")
N_STATS = 8
EVENT_STATS = ("invalid", "out_of_group", "no_decode")
RESULT_FIELDS = ("cells", "cells_roll", "sum_us", "sum_us_roll", "q_win", "q_roll", "stats")
# what WindowPipeline.results() gains with the tracker on
RESULT_KEYS = ("decode_cells", "decode_cells_roll", "decode_sum_ms", "decode_sum_ms_roll", "decode_q", "decode_q_roll")
STATE_WORDS = K + N_CELLS + 2


def stats_dict(stats: np.ndarray) -> Dict[str, int]:
    return {name: int(stats[i]) for i, name in enumerate(STATS)}


def bucket_of(u) -> np.ndarray:
    """The bucket (0..K-1) of every TPOT in ``u`` (integers in 0 .. 2^24 - 1; int64, ``u``'s shape)."""
    x = np.asarray(u).astype(np.int64)
    e = np.frexp(np.maximum(x, 1).astype(np.float64))[1].astype(np.int64) - 1  # floor(log2), exact below 2^53
    hi = 16 * (e - 3) + ((x >> np.maximum(e - 4, 0)) & 15)
    return np.where(x < 16, x, hi)


def lower(b) -> np.ndarray:
    """The smallest TPOT of every bucket in ``b`` (``K``: one past the last bucket's largest)."""
    x = np.asarray(b).astype(np.int64)
    return np.where(x < 16, x, (16 + (x & 15)) << np.maximum((x >> 4) - 1, 0))


def representative() -> np.ndarray:
    """float64 [K]: the microseconds a bucket index stands for, the midpoint of the integers it holds."""
    lo = lower(np.arange(K + 1))
    return 0.5 * (lo[:-1] + (lo[1:] - 1)).astype(np.float64)


def tpot_slo_us(tpot_slo_ms: float) -> int:
    return int(min(TPOT_MAX, max(1, int(min(float(tpot_slo_ms), 1e9) * 1000.0 + 0.5))))


def _to_ms(q: np.ndarray) -> np.ndarray:
    q = np.asarray(q).astype(np.int64)
    return np.where(q == EMPTY, np.nan, representative()[np.minimum(q, K - 1)] * 1e-3)


def quantiles_ms(result: Dict[str, np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """(window, rolling) TPOT quantiles [G, 4] in ms of a step's results; NaN for an empty service."""
    return _to_ms(result["q_win"]), _to_ms(result["q_roll"])


def result_keys(result: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """A step's results under the names WindowPipeline.results() carries (RESULT_KEYS)."""
    qw, qr = quantiles_ms(result)
    return {"decode_cells": np.asarray(result["cells"]), "decode_cells_roll": np.asarray(result["cells_roll"]),
            "decode_sum_ms": np.asarray(result["sum_us"]).astype(np.float64) * 1e-3,
            "decode_sum_ms_roll": np.asarray(result["sum_us_roll"]).astype(np.float64) * 1e-3,
            "decode_q": qw, "decode_q_roll": qr}


def empty_result(n_groups: int) -> Dict[str, np.ndarray]:
    G = int(n_groups)
    return {"cells": np.zeros((G, N_CELLS), np.uint32), "cells_roll": np.zeros((G, N_CELLS), np.uint32),
            "sum_us": np.zeros(G, np.uint64), "sum_us_roll": np.zeros(G, np.uint64),
            "q_win": np.full((G, len(PERMILLE)), EMPTY, np.uint32), "q_roll": np.full((G, len(PERMILLE)), EMPTY, np.uint32),
            "stats": np.zeros(N_STATS, np.uint32)}


def summary(cells, sum_ms, q_ms) -> Dict[str, object]:
    """One service's table, sum (ms) and quantiles (ms) as the decision log carries them; ``None``
    where there is no request."""
    c = [int(x) for x in cells]
    n = sum(c)
    tp = {name: (None if n == 0 or not np.isfinite(q_ms[j]) else round(float(q_ms[j]), 4))
          for j, name in enumerate(("p50", "p90", "p95", "p99"))}
    tp["mean"] = None if n == 0 else round(float(sum_ms) / n, 4)
    return {"requests": n, "good": c[0], "goodput": None if n == 0 else round(c[0] / n, 6), "ttft_only": c[1],
            "tpot_only": c[2], "both": c[3], "tpot_ms": tp}


# ---- layout and checks (ops/csrc/decodesli_host.h) ------------------------------------------------
def layout(group_cap: int) -> Dict[str, int]:
    """Word offsets of the result block's arrays (every array on 16 bytes) and its ``words``."""
    g = int(group_cap)
    pair = (2 * g + 3) & ~3
    off, at = {}, 0
    for name, n in (("cells", 4 * g), ("cells_roll", 4 * g), ("sum_us", pair), ("sum_us_roll", pair), ("q_win", 4 * g),
                    ("q_roll", 4 * g), ("stats", N_STATS)):
        off[name] = at
        at += n
    off["words"] = at
    return off


def device_bytes(span_cap: int, group_cap: int, windows: int) -> int:
    return int(span_cap) * 64 + (int(windows) + 2) * int(group_cap) * STATE_WORDS * 4 + layout(group_cap)["words"] * 4


def check_config(span_cap: int, group_cap: int, windows: int, n_buffers: int, slo_ms: float, tpot_slo_ms: float) -> None:
    """The configuration checks of ops/csrc/decodesli_host.h validate()."""
    if not 1 <= windows <= 4096:
        raise ValueError("decode sli: windows must be in [1, 4096]")
    if not 1 <= group_cap <= 65536:
        raise ValueError("decode sli: group_cap must be in [1, 65536]")
    if span_cap < 1:
        raise ValueError("decode sli: span_cap must be >= 1")
    if span_cap * windows >= 1 << 32:
        raise ValueError("decode sli: span_cap * windows must stay below 2^32 (a rolling counter would wrap)")
    if not 1 <= n_buffers <= 64:
        raise ValueError("decode sli: n_buffers out of range")
    if not (np.isfinite(slo_ms) and slo_ms >= 0):
        raise ValueError("decode sli: slo_ms must be finite and >= 0")
    if not (np.isfinite(tpot_slo_ms) and tpot_slo_ms > 0):
        raise ValueError("decode sli: tpot_slo_ms must be finite and > 0")
    if device_bytes(span_cap, group_cap, windows) > 1 << 31:
        raise ValueError("decode sli: the horizon needs more than 2 GiB")


def block_of(result: Dict[str, np.ndarray], group_cap: int) -> np.ndarray:
    """A step's results over all ``group_cap`` rows as the device's result block (uint32 words)."""
    off = layout(group_cap)
    out = np.zeros(off["words"], np.uint32)
    for name in RESULT_FIELDS:
        a = np.ascontiguousarray(result[name])
        w = a.view(np.uint32).reshape(-1)
        out[off[name]:off[name] + len(w)] = w
    return out


def _gather(ranges) -> np.ndarray:
    from .cpu import _gather as g

    b = g(ranges)
    return b.view(records.SPAN) if len(b) else np.zeros(0, records.SPAN)


class DecodeSliOracle(OracleCheckpoint):
    """The tracker's rules in numpy (see the module docstring), with the device handle's interface."""

    # checkpoint (pipeline/trackerstate.py): the fields ops/csrc/decodesli_host.h fingerprint() covers, and what is
    # kept between steps
    KIND = "decode sli"
    FINGERPRINT = ("group_cap", "windows", "slo_ms", "tpot_slo_ms")
    STATE = ("roll", "cells_roll", "sum_roll", "held", "n")

    def __init__(self, span_cap: int = 16384, group_cap: int = 64, windows: int = 150, n_buffers: int = 3,
                 slo_ms: float = 800.0, tpot_slo_ms: float = 100.0, device: int = 0, lds: bool = True):
        span_cap, group_cap, windows, n_buffers = int(span_cap), int(group_cap), int(windows), int(n_buffers)
        check_config(span_cap, group_cap, windows, n_buffers, float(slo_ms), float(tpot_slo_ms))
        self.span_cap, self.group_cap, self.windows, self.nb = span_cap, group_cap, windows, n_buffers
        self.slo_ms, self.tpot_slo_ms, self.tpot_slo_us = float(slo_ms), float(tpot_slo_ms), tpot_slo_us(tpot_slo_ms)
        self.roll = np.zeros((group_cap, K), np.int64)
        self.cells_roll = np.zeros((group_cap, N_CELLS), np.int64)
        self.sum_roll = np.zeros(group_cap, np.uint64)
        self.held: Dict[int, Tuple[np.ndarray, np.ndarray, np.ndarray]] = {}  # step % windows -> that step's rows
        self.res: Dict[int, Tuple[int, dict]] = {}
        self.n = 0

    # ---- one window ---------------------------------------------------------------------------
    def step(self, span_ranges: Sequence[Tuple[int, int]], n_groups: int) -> int:
        """``span_ranges`` = [(host address, bytes)] of 64-byte SPAN records, as the engine gets them."""
        for a, nbytes in span_ranges:
            if int(nbytes) % 64:
                raise ValueError("decode sli step: a range is not whole 64-byte spans")
            if int(nbytes) and not int(a):
                raise ValueError("decode sli step: null range")
        return self.step_records(_gather(span_ranges), n_groups)

    def step_records(self, spans: np.ndarray, n_groups: int) -> int:
        G, C = int(n_groups), self.group_cap
        if not 0 <= G <= C:
            raise ValueError("decode sli step: n_groups out of range")
        if len(spans) > self.span_cap:
            raise ValueError("decode sli step: more spans than span_cap")
        # nothing has changed up to here
        fl = spans["flags"].astype(np.uint32)
        grp = spans["group_id"].astype(np.int64)
        v = np.ascontiguousarray(spans["ttft_ms"], dtype=np.float32)
        u = records.span_tpot_us(fl).astype(np.int64)
        final = (fl & np.uint32(SKIP)) == 0
        has = final & (u != 0)
        ingrp = has & (grp < G)
        with np.errstate(invalid="ignore"):
            ok = ingrp & (v >= np.float32(0.0))
        g, x, t = grp[ok], u[ok], v[ok]
        hist = np.zeros((C, K), np.int64)
        np.add.at(hist, (g, bucket_of(x)), 1)
        cell = (t > np.float32(self.slo_ms)).astype(np.int64) + 2 * (x > self.tpot_slo_us).astype(np.int64)
        cells = np.zeros((C, N_CELLS), np.int64)
        np.add.at(cells, (g, cell), 1)
        sums = np.zeros(C, np.uint64)
        np.add.at(sums, g, x.astype(np.uint64))
        stats = np.zeros(N_STATS, np.uint32)
        stats[:len(STATS)] = [int(ok.sum()), int((ingrp & ~ok).sum()), int((has & ~ingrp).sum()), int((final & ~has).sum())]
        idx = self.n
        slot = idx % self.windows
        old = self.held.get(slot)
        if old is not None:
            self.roll -= old[0]
            self.cells_roll -= old[1]
            self.sum_roll -= old[2]
        self.roll += hist
        self.cells_roll += cells
        self.sum_roll += sums
        self.held[slot] = (hist, cells, sums)
        res = {"cells": cells.astype(np.uint32), "cells_roll": self.cells_roll.astype(np.uint32), "sum_us": sums,
               "sum_us_roll": self.sum_roll.copy(), "q_win": rank_buckets(hist), "q_roll": rank_buckets(self.roll),
               "stats": stats}
        self.res[idx % self.nb] = (idx, res)
        self.n += 1
        return idx

    # ---- results ------------------------------------------------------------------------------
    def query(self, i: int) -> bool:
        return True

    def _held(self, i: int) -> dict:
        held = self.res.get(int(i) % self.nb)
        if held is None or held[0] != int(i):
            raise IndexError(f"decode sli step {i} is not held (only the last {self.nb})")
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
        """The rolling state: ``rows`` [group_cap, K], ``cells`` [group_cap, 4], ``sum_us`` [group_cap] and
        ``pos``, the horizon row the next step replaces."""
        return {"rows": self.roll.astype(np.uint32), "cells": self.cells_roll.astype(np.uint32),
                "sum_us": self.sum_roll.copy(), "pos": self.n % self.windows}

    def sync(self) -> None:
        pass

    def close(self) -> None:
        pass
