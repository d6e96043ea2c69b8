"""Open-request tracking on the host: the agent as the TTFT deadline clock.

A service exports a start record when a request starts (collector/records.py SPAN_START: a SPAN
with ``flags = SPAN_START | SPAN_NO_SLI``, ``ttft_ms`` NaN, ``ts_ns`` the request start). The
tracker keeps the open requests and, at every window cut, counts the requests whose
``start + SLO`` has passed with no SLI record yet -- once -- and takes them out of the window their
late record finally lands in. The window engines are not touched: the tracker produces per-group
corrections to their ``sli`` / ``late`` counts (``correct_results``).

``OpenRequestOracle`` is the rules in plain Python over a dict: the reference the device table
(ops/csrc/openreq.hip, ops/openreq.py) is tested against, and what ``engine="cpu"`` uses.

Per step (one window), in this order:

1. insert -- every record with SPAN_START, ``trace_h != 0``, ``ts_ns > 0`` and ``group_id <
   n_groups``: no entry -> OPEN; an OPEN / COUNTED entry -> ``dup_start``; a RESOLVED marker ->
   the start is dropped (``start_after_sli``); no room -> ``dropped_full``.
2. resolve -- every record the engine counts (no SPAN_START, no SPAN_NO_SLI, ``trace_h != 0``):
   OPEN -> removed; COUNTED -> removed, and the engine's count of this record is taken back:
   ``dup[g][2]`` if it breaches and carries SPAN_LATE, else ``dup[g][0]`` (and ``dup[g][1]`` if it
   breaches), ``g`` the record's group; a record within the SLO after all -> ``false_deadline``;
   no entry -> a RESOLVED marker born at this cut.
3. sweep -- OPEN with ``start + slo < cut`` -> ``dl[g][0]`` if the deadline is >= the previous cut,
   else ``dl[g][1]`` (an earlier window's breach, like SPAN_LATE), and COUNTED; COUNTED with
   ``cut - start >= ttl`` -> removed (``expired``); a marker with ``cut - born >= reorder`` ->
   removed. The state a row had when the sweep reached it decides: one transition per step.

The service's start time and the agent's cut time are compared directly (same-node clocks).
"""

from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

from ..collector import records
from .trackerstate import OracleCheckpoint

OPEN, COUNTED, RESOLVED = 1, 2, 3
STATE_NAMES = {OPEN: "open", COUNTED: "counted", RESOLVED: "resolved"}
# per-step statistics, in the device's order (ops/csrc/openreq_host.h Stat)
STATS = ("dup_start", "start_after_sli", "dropped_full", "expired", "false_deadline", "live_open", "live_counted",
         "live_resolved", "starts", "resolves", "marker_dropped")
N_STATS = 16
EVENT_STATS = ("dup_start", "start_after_sli", "dropped_full", "expired", "false_deadline")
MAX_PROBES = 64
RESULT_KEYS = ("sli_raw", "late_raw", "deadline", "deadline_dup")


def stats_dict(stats: np.ndarray) -> Dict[str, int]:
    return {name: int(stats[i]) for i, name in enumerate(STATS)}


def ms_to_ns(ms: float) -> int:
    return int(round(float(ms) * 1e6))


def unordered_traces(spans: np.ndarray) -> int:
    """Traces with more than one counted record in the window: which of them removes the entry is
    unordered on the device (the inputs of an equality test must hold none)."""
    fl = spans["flags"]
    counted = ((fl & np.uint32(records.SPAN_START | records.SPAN_NO_SLI)) == 0) & (spans["trace_h"] != 0)
    _, n = np.unique(spans["trace_h"][counted], return_counts=True)
    return int((n > 1).sum())


def correct_results(res: Dict[str, np.ndarray], tr: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """The engine's per-group results with the tracker's corrections applied: ``sli`` / ``late``
    corrected, the engine's own as ``sli_raw`` / ``late_raw``, the tracker's ``deadline`` (dl) and
    ``deadline_dup`` (dup)."""
    out = dict(res)
    sli, late = np.asarray(res["sli"]), np.asarray(res["late"])
    G = sli.shape[0]
    dl = np.zeros((G, 2), np.int64)
    dup = np.zeros((G, 3), np.int64)
    n = min(G, len(tr["dl"]))
    dl[:n], dup[:n] = tr["dl"][:n], tr["dup"][:n]
    s = sli.astype(np.int64)
    s[:, 0] += dl[:, 0] - dup[:, 0]
    s[:, 1] += dl[:, 0] - dup[:, 1]
    la = late.astype(np.int64)
    la[:, 0] += dl[:, 1] - dup[:, 2]
    out["sli_raw"], out["late_raw"] = sli, late
    out["sli"] = np.maximum(s, 0).astype(sli.dtype)
    out["late"] = np.maximum(la, 0).astype(late.dtype)
    out["deadline"] = dl.astype(np.uint32)
    out["deadline_dup"] = dup.astype(np.uint32)
    return out


def _gather(ranges) -> np.ndarray:
    from .cpu import _gather as g

    b = g(ranges)
    return b.view(records.SPAN) if len(b) else np.zeros(0, records.SPAN)


class OpenRequestOracle(OracleCheckpoint):
    """The tracker's rules over a dict (see the module docstring). ``cap`` bounds the rows a step
    may hold, removed ones included: the device's table probes at most MAX_PROBES slots, which is
    the whole table at ``cap`` <= MAX_PROBES (there the two agree on ``dropped_full``); a larger
    device table can also drop a start whose probe run is full while the table is not."""

    # checkpoint (pipeline/trackerstate.py): the fields ops/csrc/openreq_host.h fingerprint() covers, and what is
    # kept between steps
    KIND = "open-request"
    FINGERPRINT = ("cap", "group_cap", "slo_ms", "ttl_ns", "reorder_ns")
    STATE = ("tab", "n")

    def __init__(self, cap: int = 1 << 20, span_cap: int = 16384, group_cap: int = 64, n_buffers: int = 3,
                 slo_ms: float = 800.0, ttl_ms: float = 120000.0, reorder_ms: float = 2000.0, device: int = 0):
        if cap < MAX_PROBES or cap & (cap - 1):
            raise ValueError("cap must be a power of two >= 64")
        self.cap, self.span_cap, self.group_cap, self.nb = int(cap), int(span_cap), int(group_cap), int(n_buffers)
        self.slo_ms = float(slo_ms)
        self.slo_ns, self.ttl_ns, self.reorder_ns = ms_to_ns(slo_ms), ms_to_ns(ttl_ms), ms_to_ns(reorder_ms)
        self.tab: Dict[int, List[int]] = {}  # trace_h -> [t, grp, state]
        self.res: Dict[int, Tuple[int, dict]] = {}
        self.n = 0

    # ---- one window ---------------------------------------------------------------------------
    def step(self, span_ranges: Sequence[Tuple[int, int]], cut_ns: int, prev_cut_ns: int, n_groups: int) -> int:
        """``span_ranges`` = [(host address, bytes)] of 64-byte SPAN records, as the engine gets them."""
        return self.step_records(_gather(span_ranges), cut_ns, prev_cut_ns, n_groups)

    def step_records(self, spans: np.ndarray, cut_ns: int, prev_cut_ns: int, n_groups: int) -> int:
        cut, prev, G = int(cut_ns), int(prev_cut_ns), int(n_groups)
        if cut <= 0 or not 0 <= prev <= cut or not 0 <= G <= self.group_cap:
            raise ValueError("open-request step: cut / prev_cut / n_groups out of range")
        if len(spans) > self.span_cap:
            raise ValueError("open-request step: more spans than span_cap")
        dl, dup = np.zeros((G, 2), np.uint32), np.zeros((G, 3), np.uint32)
        st = dict.fromkeys(STATS, 0)
        tab = self.tab
        fl = spans["flags"].astype(np.int64)
        th = spans["trace_h"].astype(np.uint64)
        ts, grp, ttft = spans["ts_ns"].astype(np.int64), spans["group_id"].astype(np.int64), spans["ttft_ms"]
        dead = 0  # rows removed in this step still hold their slot until its end
        is_start = (fl & records.SPAN_START) != 0
        for i in np.nonzero(is_start & (th != 0) & (grp < G) & (ts > 0))[0].tolist():
            st["starts"] += 1
            e = tab.get(int(th[i]))
            if e is None:
                if len(tab) + dead >= self.cap:
                    st["dropped_full"] += 1
                else:
                    tab[int(th[i])] = [int(ts[i]), int(grp[i]), OPEN]
            elif e[2] == RESOLVED:
                st["start_after_sli"] += 1
            else:
                st["dup_start"] += 1
        slo = np.float32(self.slo_ms)
        for i in np.nonzero(~is_start & ((fl & records.SPAN_NO_SLI) == 0) & (th != 0))[0].tolist():
            st["resolves"] += 1
            key = int(th[i])
            e = tab.get(key)
            if e is None:
                if len(tab) + dead >= self.cap:
                    st["marker_dropped"] += 1
                else:
                    tab[key] = [cut, int(grp[i]), RESOLVED]
            elif e[2] == OPEN:
                del tab[key]
                dead += 1
            elif e[2] == COUNTED:
                del tab[key]
                dead += 1
                breach = bool(ttft[i] > slo)
                g = int(grp[i])
                if g < G:  # the engine counted the record in this group
                    if breach and fl[i] & records.SPAN_LATE:
                        dup[g, 2] += 1
                    else:
                        dup[g, 0] += 1
                        dup[g, 1] += int(breach)
                if not breach:
                    st["false_deadline"] += 1
        for key in list(tab):
            t, g, s = tab[key]
            if s == OPEN:
                if t + self.slo_ns < cut:
                    if g < G:
                        dl[g, 0 if t + self.slo_ns >= prev else 1] += 1
                    tab[key][2] = COUNTED
            elif s == COUNTED:
                if cut - t >= self.ttl_ns:
                    del tab[key]
                    st["expired"] += 1
            elif cut - t >= self.reorder_ns:
                del tab[key]
        for e in tab.values():
            st["live_" + STATE_NAMES[e[2]]] += 1
        stats = np.zeros(N_STATS, np.uint32)
        stats[:len(STATS)] = [st[k] for k in STATS]
        idx = self.n
        self.res[idx % self.nb] = (idx, {"dl": dl, "dup": dup, "stats": stats})
        self.n += 1
        return idx

    # ---- results ------------------------------------------------------------------------------
    def query(self, i: int) -> bool:
        return True

    def results(self, i: int, n_groups: int) -> Dict[str, np.ndarray]:
        held = self.res.get(int(i) % self.nb)
        if held is None or held[0] != int(i):
            raise KeyError(f"open-request step {i} is not held (only the last {self.nb})")
        r = held[1]
        G = int(n_groups)
        dl, dup = np.zeros((G, 2), np.uint32), np.zeros((G, 3), np.uint32)
        n = min(G, len(r["dl"]))
        dl[:n], dup[:n] = r["dl"][:n], r["dup"][:n]
        return {"dl": dl, "dup": dup, "stats": r["stats"].copy()}

    def step_ms(self, i: int) -> Tuple[float, float]:
        return 0.0, 0.0

    def entries(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The live rows (trace_h, t, grp, state), sorted by trace hash."""
        keys = sorted(self.tab)
        rows = [self.tab[k] for k in keys]
        return (np.array(keys, dtype=np.uint64), np.array([r[0] for r in rows], dtype=np.int64),
                np.array([r[1] for r in rows], dtype=np.uint32), np.array([r[2] for r in rows], dtype=np.uint32))

    def probe_lengths(self) -> np.ndarray:
        """Probes each live row needs when the rows enter an empty table of ``cap`` slots in key
        order (splitmix64 home slot, linear probing): the device table's chains, up to order."""
        mask = self.cap - 1
        used = set()
        out = []
        for k in sorted(self.tab):
            s = splitmix64(k) & mask
            n = 1
            while s in used and n <= self.cap:
                s = (s + 1) & mask
                n += 1
            used.add(s)
            out.append(n)
        return np.array(out, dtype=np.int64)

    def sync(self) -> None:
        pass

    def close(self) -> None:
        pass


def splitmix64(x: int) -> int:
    """ops/csrc/mislo_common.h splitmix64."""
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)
