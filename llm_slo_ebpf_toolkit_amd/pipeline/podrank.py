"""Per-pod TTFT breach breakdown per service on the host: the rules of the pod-breakdown tracker.

``sli[g] = (requests, breaches)`` says how bad a service is, not where: one throttled replica and a
service-wide stall look the same. Per step (one window, the span ranges the engine gets) the tracker
yields, per service (incident group) and for two scopes --

* **window** (``win_*``): this step only,
* **recent** (``rec_*``): the last ``H`` steps, this one included (the horizon is counted in steps:
  every step ages every row of ``group_cap``, whether or not the group is present) --

``n`` / ``b`` (observed requests and breaches, exact), ``pods`` / ``pods_b`` (distinct pods seen, and
those with at least one breach), and ``k_top`` / ``top[K]``: the K pods with the most breaches as
32-byte rows (``POD_ROW``: the pod's requests, breaches, largest TTFT and exact TTFT sum).

``PodRankOracle`` is the rules in numpy: the reference the device tracker (ops/csrc/podrank.hip,
ops/podrank.py) is tested against for equality, and what ``engine="cpu"`` uses.

**Which records count**: the sketch's observed set. A 64-byte SPAN without SPAN_NO_SLI, with
``group_id < n_groups`` and ``ttft_ms >= 0`` in a float32 compare; NaN and negatives are ``invalid``,
groups at or above ``n_groups`` are ``out_of_group``, SPAN_LATE records count by their value. An
observed record with ``pod_id >= 2^20`` counts in ``n`` / ``b`` but in no pod row
(``pod_out_of_range``); pod 0, the unknown pod, is an ordinary pod.

**Breach**: ``ttft_ms > slo_ms`` in float32 (the engine's compare); equal is no breach, +inf is one.

**Per pair** (service, pod): ``n``, ``b``, ``max`` of ``ord(v) = float bits & 0x7fffffff`` and the
sum of ``milli_units(min(v, 2^21))`` in 64 bits -- integers only, so every result is exact.

**Ranking**: pairs with ``b >= 1`` only; more breaches first, then fewer requests (the higher breach
share), then the lower pod id: ``key = b << 42 | (2^22 - 1 - n) << 20 | (2^20 - 1 - pod)``.

**Capacity**: a window holds at most ``pair_cap`` distinct pairs. Beyond that which pairs are kept is
unspecified (this oracle keeps the first in record order and reports the step as ``overflowed``);
the records of the others go to ``pair_overflow``, ``n`` / ``b`` stay exact.
"""

from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

from ..collector import records
from .trackerstate import OracleCheckpoint
from .oracle import milli_units

MAX_K = 8
MAX_H = 16
POD_LIMIT = 1 << 20
COUNT_LIMIT = 1 << 22
MAX_PAIR_CAP = 1 << 20
MAX_MS = 2097152.0           # 2^21, the sum's clamp
ROW_BYTES = 32
ENTRY_BYTES = 28             # a table or list entry on the device: key, n, b, max, sum
# one ranked pod (ops/csrc/podrank_host.h Row)
POD_ROW = np.dtype([("pod_id", "<u4"), ("n", "<u4"), ("b", "<u4"), ("max_ttft", "<f4"), ("sum_milli", "<u8"),
                    ("pad", "<u4", (2,))])
assert POD_ROW.itemsize == ROW_BYTES
# one resident pair of the horizon's lists
PAIR = np.dtype([("g", "<u4"), ("pod", "<u4"), ("n", "<u4"), ("b", "<u4"), ("max_bits", "<u4"), ("sum_milli", "<u8")])
# per-step statistics, in the device's order (ops/csrc/podrank_host.h Stat)
STATS = ("observed", "invalid", "out_of_group", "pod_out_of_range", "pair_overflow")
N_STATS = 8
EVENT_STATS = ("invalid", "out_of_group", "pod_out_of_range", "pair_overflow")
SCOPES = ("win", "rec")
SCOPE_FIELDS = ("n", "b", "pods", "pods_b", "k_top", "top")
RESULT_FIELDS = tuple(f"{s}_{f}" for s in SCOPES for f in SCOPE_FIELDS) + ("stats",)
# what WindowPipeline.results() gains with the tracker on
RESULT_KEYS = tuple(f"pod_{f}" for f in RESULT_FIELDS if f != "stats")

_M64 = (1 << 64) - 1


def stats_dict(stats: np.ndarray) -> Dict[str, int]:
    return {name: int(stats[i]) for i, name in enumerate(STATS)}


def fmix64(x: int) -> int:
    """murmur3's 64-bit finalizer."""
    x &= _M64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & _M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & _M64
    x ^= x >> 33
    return x


def pair_key(g: int, pod: int) -> int:
    return ((int(g) + 1) << 32) | int(pod)


def slot_of(g: int, pod: int, slots: int) -> int:
    """The first slot the device probes for (g, pod) in a table of ``slots`` (a power of two)."""
    return fmix64(pair_key(g, pod)) & (int(slots) - 1)


def pow2_at_least(v: int) -> int:
    p = 1
    while p < v:
        p <<= 1
    return p


def window_slots(pair_cap: int) -> int:
    return pow2_at_least(2 * int(pair_cap))


def recent_slots(pair_cap: int, windows: int) -> int:
    return pow2_at_least(2 * int(pair_cap) * int(windows))


def rank_key(b, n, pod) -> np.ndarray:
    """uint64: ``b << 42 | (2^22 - 1 - n) << 20 | (2^20 - 1 - pod)``."""
    b, n, pod = (np.asarray(a, dtype=np.uint64) for a in (b, n, pod))
    return (b << np.uint64(42)) | ((np.uint64(COUNT_LIMIT - 1) - n) << np.uint64(20)) | (np.uint64(POD_LIMIT - 1) - pod)


def rank_unpack(key) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(b, n, pod) of rank keys."""
    key = np.asarray(key, dtype=np.uint64)
    b = key >> np.uint64(42)
    n = np.uint64(COUNT_LIMIT - 1) - ((key >> np.uint64(20)) & np.uint64(COUNT_LIMIT - 1))
    pod = np.uint64(POD_LIMIT - 1) - (key & np.uint64(POD_LIMIT - 1))
    return b, n, pod


def result_keys(result: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """A step's results under the names WindowPipeline.results() carries (RESULT_KEYS)."""
    return {f"pod_{f}": np.asarray(result[f]) for f in RESULT_FIELDS if f != "stats"}


def empty_result(n_groups: int, k: int) -> Dict[str, np.ndarray]:
    G = int(n_groups)
    res: Dict[str, np.ndarray] = {}
    for s in SCOPES:
        for f in SCOPE_FIELDS[:-1]:
            res[f"{s}_{f}"] = np.zeros(G, np.uint32)
        res[f"{s}_top"] = np.zeros((G, int(k)), POD_ROW)
    res["stats"] = np.zeros(N_STATS, np.uint32)
    return res


def layout_words(group_cap: int, k: int) -> int:
    g4 = (int(group_cap) + 3) & ~3
    at = 10 * g4 + 2 * int(group_cap) * int(k) * (ROW_BYTES // 4) + N_STATS
    return (at + 3) & ~3


def device_bytes(k: int, windows: int, pair_cap: int, span_cap: int, group_cap: int) -> int:
    """ops/csrc/podrank_host.h device_bytes()."""
    G, H = int(group_cap), int(windows)
    return (span_cap * 64 + (window_slots(pair_cap) + recent_slots(pair_cap, H)) * ENTRY_BYTES
            + H * pair_cap * ENTRY_BYTES + (2 + 2 * H) * G * 4 + 2 * G * k * 8 + layout_words(G, k) * 4 + (H + 1) * 4)


def check_config(k: int, windows: int, pair_cap: int, span_cap: int, group_cap: int, n_buffers: int,
                 slo_ms: float) -> None:
    """The configuration checks of ops/csrc/podrank_host.h validate()."""
    if not 1 <= k <= MAX_K:
        raise ValueError("pod breakdown: k must be in [1, 8]")
    if not 1 <= windows <= MAX_H:
        raise ValueError("pod breakdown: windows must be in [1, 16]")
    if not 1 <= pair_cap <= MAX_PAIR_CAP:
        raise ValueError("pod breakdown: pair_cap must be in [1, 2^20]")
    if not 1 <= group_cap <= 65536:
        raise ValueError("pod breakdown: group_cap must be in [1, 65536]")
    if span_cap < 1 or span_cap * windows >= COUNT_LIMIT:
        raise ValueError("pod breakdown: span_cap must be >= 1 and span_cap * windows < 2^22")
    if not 1 <= n_buffers <= 64:
        raise ValueError("pod breakdown: n_buffers out of range")
    if not (np.isfinite(slo_ms) and slo_ms >= 0):
        raise ValueError("pod breakdown: slo_ms must be finite and >= 0")
    if device_bytes(k, windows, pair_cap, span_cap, group_cap) > 1 << 31:
        raise ValueError("pod breakdown: the tables need more than 2 GiB")


def _gather(ranges) -> np.ndarray:
    from .cpu import _gather as g

    b = g(ranges)
    return b.view(records.SPAN) if len(b) else np.zeros(0, records.SPAN)


def sort_pairs(pairs: np.ndarray) -> np.ndarray:
    """A resident list in the order tests compare it in: by (g, pod)."""
    return pairs[np.lexsort((pairs["pod"], pairs["g"]))]


def merge_pairs(lists: Sequence[np.ndarray]) -> np.ndarray:
    """The pairs of several lists under one key each: counts and sums added, the larger maximum."""
    allp = np.concatenate([np.asarray(l, PAIR) for l in lists]) if len(lists) else np.zeros(0, PAIR)
    if not len(allp):
        return np.zeros(0, PAIR)
    key = ((allp["g"].astype(np.uint64) + np.uint64(1)) << np.uint64(32)) | allp["pod"].astype(np.uint64)
    uniq, inv = np.unique(key, return_inverse=True)
    out = np.zeros(len(uniq), PAIR)
    out["g"] = ((uniq >> np.uint64(32)) - np.uint64(1)).astype(np.uint32)
    out["pod"] = (uniq & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    for f in ("n", "b"):
        acc = np.zeros(len(uniq), np.int64)
        np.add.at(acc, inv, allp[f].astype(np.int64))
        out[f] = acc
    mx = np.zeros(len(uniq), np.uint32)
    np.maximum.at(mx, inv, allp["max_bits"])
    out["max_bits"] = mx
    sm = np.zeros(len(uniq), np.uint64)
    np.add.at(sm, inv, allp["sum_milli"])
    out["sum_milli"] = sm
    return out


def scope_of(pairs: np.ndarray, group_cap: int, k: int) -> Dict[str, np.ndarray]:
    """``pods`` / ``pods_b`` / ``k_top`` / ``top`` of one scope's pairs."""
    C, K = int(group_cap), int(k)
    g = pairs["g"].astype(np.int64)
    hot = pairs["b"] >= 1
    top = np.zeros((C, K), POD_ROW)
    k_top = np.zeros(C, np.uint32)
    hp = pairs[hot]
    if len(hp):
        key = rank_key(hp["b"], hp["n"], hp["pod"])
        by_key = np.argsort(key)[::-1]
        order = by_key[np.argsort(hp["g"][by_key], kind="stable")]
        gs = hp["g"][order].astype(np.int64)
        cnt = np.bincount(gs, minlength=C)
        first = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
        pos = np.arange(len(gs)) - first[gs]
        keep = pos < K
        rows = np.zeros(int(keep.sum()), POD_ROW)
        src = hp[order[keep]]
        rows["pod_id"], rows["n"], rows["b"], rows["sum_milli"] = src["pod"], src["n"], src["b"], src["sum_milli"]
        rows["max_ttft"] = np.ascontiguousarray(src["max_bits"]).view(np.float32)
        top[gs[keep], pos[keep]] = rows
        k_top = np.minimum(cnt, K).astype(np.uint32)
    return {"pods": np.bincount(g, minlength=C).astype(np.uint32),
            "pods_b": np.bincount(g[hot], minlength=C).astype(np.uint32), "k_top": k_top, "top": top}


class PodRankOracle(OracleCheckpoint):
    """The tracker's rules in numpy (see the module docstring), with the device handle's interface."""

    # checkpoint (pipeline/trackerstate.py): the fields ops/csrc/podrank_host.h fingerprint() covers, and what is
    # kept between steps
    KIND = "pod breakdown"
    FINGERPRINT = ("group_cap", "windows", "k", "pair_cap", "slo_ms")
    STATE = ("lists", "hist", "n")

    def __init__(self, k: int = 3, windows: int = 3, pair_cap: int = 4096, span_cap: int = 16384, group_cap: int = 64,
                 n_buffers: int = 3, slo_ms: float = 800.0, device: int = 0):
        k, windows, pair_cap, span_cap = int(k), int(windows), int(pair_cap), int(span_cap)
        group_cap, n_buffers, slo_ms = int(group_cap), int(n_buffers), float(slo_ms)
        check_config(k, windows, pair_cap, span_cap, group_cap, n_buffers, slo_ms)
        self.k, self.windows, self.pair_cap, self.span_cap = k, windows, pair_cap, span_cap
        self.group_cap, self.nb, self.slo_ms = group_cap, n_buffers, slo_ms
        self.lists: List[np.ndarray] = [np.zeros(0, PAIR) for _ in range(windows)]  # slot step % windows
        self.hist = np.zeros((windows, 2, group_cap), np.uint32)                    # n, b of the horizon's steps
        self.res: Dict[int, Tuple[int, dict, bool]] = {}
        self.n = 0

    # ---- one window ---------------------------------------------------------------------------
    def step(self, span_ranges: Sequence[Tuple[int, int]], n_groups: int) -> int:
        """``span_ranges`` = [(host address, bytes)] of 64-byte SPAN records, as the engine gets them."""
        for _a, nbytes in span_ranges:
            if int(nbytes) % 64:
                raise ValueError("pod breakdown step: a range is not whole 64-byte spans")
        return self.step_records(_gather(span_ranges), n_groups)

    def step_records(self, spans: np.ndarray, n_groups: int) -> int:
        G, C, K, H = int(n_groups), self.group_cap, self.k, self.windows
        if not 0 <= G <= C:
            raise ValueError("pod breakdown step: n_groups out of range")
        if len(spans) > self.span_cap:
            raise ValueError("pod breakdown step: more spans than span_cap")
        grp = spans["group_id"].astype(np.int64)
        v = np.ascontiguousarray(spans["ttft_ms"], dtype=np.float32)
        sli = (spans["flags"] & np.uint32(records.SPAN_NO_SLI)) == 0
        counts = sli & (grp < G)
        with np.errstate(invalid="ignore"):
            ok = counts & (v >= np.float32(0.0))
        at = np.nonzero(ok)[0]
        g, pod, x = grp[at], spans["pod_id"][at].astype(np.int64), v[at]
        breach = x > np.float32(self.slo_ms)
        n_tot = np.bincount(g, minlength=C).astype(np.uint32)
        b_tot = np.bincount(g[breach], minlength=C).astype(np.uint32)
        inr = pod < POD_LIMIT
        # the pairs, in the order of their first record
        key = ((g[inr].astype(np.uint64) + np.uint64(1)) << np.uint64(32)) | pod[inr].astype(np.uint64)
        uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
        seen = np.empty(len(uniq), np.int64)
        seen[np.argsort(first, kind="stable")] = np.arange(len(uniq))
        kept = seen < self.pair_cap
        overflowed = len(uniq) > self.pair_cap
        pairs = np.zeros(len(uniq), PAIR)
        pairs["g"] = ((uniq >> np.uint64(32)) - np.uint64(1)).astype(np.uint32)
        pairs["pod"] = (uniq & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        pairs["n"] = np.bincount(inv, minlength=len(uniq))
        pairs["b"] = np.bincount(inv[breach[inr]], minlength=len(uniq))
        mx = np.zeros(len(uniq), np.uint32)
        np.maximum.at(mx, inv, np.ascontiguousarray(x[inr]).view(np.uint32) & np.uint32(0x7FFFFFFF))
        pairs["max_bits"] = mx
        sm = np.zeros(len(uniq), np.uint64)
        np.add.at(sm, inv, milli_units(np.minimum(x[inr], np.float32(MAX_MS))).astype(np.uint64))
        pairs["sum_milli"] = sm
        stats = np.zeros(N_STATS, np.uint32)
        stats[:len(STATS)] = [len(at), int((counts & ~ok).sum()), int((sli & (grp >= G)).sum()), int((~inr).sum()),
                              int(pairs["n"][~kept].sum())]
        pairs = pairs[kept]

        idx = self.n
        cur = idx % H
        self.lists[cur] = pairs
        self.hist[cur, 0], self.hist[cur, 1] = n_tot, b_tot
        res: Dict[str, np.ndarray] = {"win_n": n_tot, "win_b": b_tot, "rec_n": self.hist[:, 0].sum(axis=0, dtype=np.uint32),
                                      "rec_b": self.hist[:, 1].sum(axis=0, dtype=np.uint32), "stats": stats}
        for s, p in (("win", pairs), ("rec", merge_pairs(self.lists))):
            for f, a in scope_of(p, C, K).items():
                res[f"{s}_{f}"] = a
        self.res[idx % self.nb] = (idx, res, overflowed)
        self.n += 1
        return idx

    # ---- results ------------------------------------------------------------------------------
    def query(self, i: int) -> bool:
        return True

    def _held(self, i: int):
        held = self.res.get(int(i) % self.nb)
        if held is None or held[0] != int(i):
            raise IndexError(f"pod breakdown step {i} is not held (only the last {self.nb})")
        return held

    def results(self, i: int, n_groups: int) -> Dict[str, np.ndarray]:
        held = self._held(i)
        G = int(n_groups)
        if not 0 <= G <= self.group_cap:
            raise ValueError("n_groups")
        return {f: (held[1][f].copy() if f == "stats" else held[1][f][:G].copy()) for f in RESULT_FIELDS}

    def overflowed(self, i: int) -> bool:
        """Step ``i`` had more distinct pairs than ``pair_cap``: which pairs were kept is unspecified."""
        return bool(self._held(i)[2])

    def step_ms(self, i: int) -> Tuple[float, float]:
        return 0.0, 0.0

    def resident(self) -> List[np.ndarray]:
        """The horizon: per slot (step % windows) its PAIR list."""
        return [p.copy() for p in self.lists]

    def sync(self) -> None:
        pass

    def close(self) -> None:
        pass
