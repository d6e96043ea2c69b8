"""Hand-built join windows for the paths of ops/csrc/join.hip that replay windows never enter.

Plain numpy, no GPU: every case is a window of 64-byte EVENT / SPAN records (collector/records.py)
with the incident-group count and the join parameter sets to run it with. ``oracle.join_bruteforce``
is the reference for all of them; tests/test_join_cases.py checks on the reference output alone that
each case still contains what it was built for, tests/test_join_edges_gpu.py runs them on the GPU.

Timestamps sit around a fixed epoch, rows are given in shuffled input order (the join's last
tie-break is input order), the event ``conn_h`` is set directly, signal types come from the
catalogue with one unsupported type (42) mixed in. At most 8192 events and 1024 spans per case.

Cases (``cases()``), with the join.hip path each one aims at:

* ``boundaries``       -- one span per tier, signals at T +- w, +- (w - 1 ns), +- (w + 1 ns) for the four
                          tier windows: the <= / < of every lower_ht / upper_ht bound and dt test, at
                          outer windows 2000, 100 (every tier clipped) and 300 ms.
* ``boundaries_wide``  -- outer window 34 s, trace pairs at |dt| = 33.9 s: the dt field of the top-3 key
                          next to the tier bits.
* ``zero_keys``        -- every subset of {trace, pod, pid, conn, svc, node, ts} zeroed on spans and
                          signals: kNoPart on both sides, equal-because-zero fields never match.
* ``precedence``       -- one identity, a signal per combination of {trace, pid, conn, svc|node} equal
                          at four |dt|: first-tier-wins, the owner / fix_low accounting of the trace
                          pass, thresholds 0.6 .. 1.5, fanout 1 .. 3, both group modes.
* ``ranking``          -- 0 .. 6 trace matches per span, the rest of the top-3 from the pod tiers (needy
                          spans), |dt| ties broken by input order, spans sharing a trace id, max-merge.
* ``mixed_runs``       -- (pod, pid) runs mixed in group / svc|node / conn, (pod, conn) runs mixed in pid
                          (s_runok == 0: the exact walk), a uniform (pod, conn) run with the pod+pid
                          sub-range, and two constructed 64-bit pod+conn hash collisions (the span list
                          holds one key / both keys).
* ``long_lists``       -- 600 spans on one (pod, pid), (pod, conn) and svc|node in 3 groups (chunks 256 +
                          256 + 88, mixed runs) and 300 spans on a second, uniform key (256 + 44).
* ``sliced_lists``     -- more than 6144 signals on one (pod, pid), one trace id and one svc|node: every
                          list is sliced into several probe items, the trace flush is not ``sole``.
* ``many_groups_65`` / ``many_groups_100`` -- more incident groups than the probe keeps in LDS, group
                          ids up to and beyond ``n_groups`` (ignored).

``halo_pair()`` is two consecutive windows for an engine with a halo: rows at the halo cut-off and
1 ns before it, and |dt| ties between rows of the two windows.
"""

from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass, field
from typing import Dict, Tuple

import numpy as np

from ..collector import records
from ..signals import catalog
from ..utils.timeutil import MS

EPOCH_NS = 1_700_000_000 * 1_000_000_000
UNSUPPORTED_TYPE = 42
MAX_EVENTS, MAX_SPANS = 8192, 1024
TIER_WINDOWS_MS = (2000, 100, 250, 500)  # trace (the default outer window), pod+pid, pod+conn, svc+node
_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_TYPES = np.array([s.kernel_type for s in catalog.SIGNALS], dtype=np.uint16)
_SCALE = {s.kernel_type: s.decode_scale for s in catalog.SIGNALS}
assert UNSUPPORTED_TYPE not in _SCALE


# ---- the key hash of ops/csrc/mislo_common.h, and a constructed collision ---------------------

def key_hash(k: int, trace: int, pod: int, pid: int, conn: int, svcnode: int) -> int:
    """Python mirror of ``key_hash`` (mislo_common.h): 0 = invalid key."""
    if k == 0:
        if trace == 0:
            return 0
        key = trace ^ 0x1111111111111111
    elif k == 1:
        if pod == 0 or pid == 0:
            return 0
        key = ((pod << 32) | pid) ^ 0x2222222222222222
    elif k == 2:
        if pod == 0 or conn == 0:
            return 0
        key = records.splitmix64(conn) ^ ((pod * _GOLDEN) & _M64) ^ 0x3333333333333333
    else:
        if (svcnode >> 16) == 0 or (svcnode & 0xFFFF) == 0:
            return 0
        key = svcnode ^ 0x4444444444444444
    return records.splitmix64(key & _M64) or 1


def _unxorshift(z: int, s: int) -> int:
    x = z
    for _ in range(64 // s + 1):
        x = z ^ (x >> s)
    return x


def splitmix64_inv(y: int) -> int:
    """The inverse of ``records.splitmix64`` (a bijection of 64-bit words)."""
    z = _unxorshift(y, 31)
    z = (z * pow(0x94D049BB133111EB, -1, 1 << 64)) & _M64
    z = _unxorshift(z, 27)
    z = (z * pow(0xBF58476D1CE4E5B9, -1, 1 << 64)) & _M64
    z = _unxorshift(z, 30)
    return (z - _GOLDEN) & _M64


def colliding_conn(pod1: int, conn1: int, pod2: int) -> int:
    """The connection that gives (pod2, conn) the pod+conn key hash of (pod1, conn1)."""
    conn2 = splitmix64_inv(records.splitmix64(conn1) ^ ((pod1 * _GOLDEN) & _M64) ^ ((pod2 * _GOLDEN) & _M64))
    assert records.splitmix64(splitmix64_inv(0x0123456789ABCDEF)) == 0x0123456789ABCDEF
    assert conn2 != 0 and (pod1, conn1) != (pod2, conn2)
    assert key_hash(2, 0, pod1, 0, conn1, 0) == key_hash(2, 0, pod2, 0, conn2, 0)
    return conn2


# ---- building a window -----------------------------------------------------------------------

@dataclass
class JoinCase:
    name: str
    events: np.ndarray            # records.EVENT, shuffled input order
    spans: np.ndarray             # records.SPAN, shuffled input order
    n_groups: int
    params: Tuple[dict, ...]      # window_ms / threshold / fanout / group_mode sets to run it with
    info: dict = field(default_factory=dict)  # what the coverage checks need (row indices after the shuffle)


def _params(window_ms=2000.0, threshold=0.7, fanout=3, group_mode=1) -> dict:
    return dict(window_ms=float(window_ms), threshold=float(threshold), fanout=int(fanout), group_mode=int(group_mode))


class _Window:
    def __init__(self, seed: int):
        self.rng = np.random.default_rng(seed)
        self.ev, self.sp = [], []
        self.n_ev = self.n_sp = 0

    def signals(self, ts, trace=0, pod=0, pid=0, conn=0, svc=0, node=0, typ=None, mix42=False) -> np.ndarray:
        """Append signals (fields broadcast against ``ts``); returns their pre-shuffle row indices."""
        ts = np.atleast_1d(np.asarray(ts, dtype=np.int64))
        n = len(ts)
        e = np.zeros(n, dtype=records.EVENT)
        e["ts_ns"], e["trace_h"], e["pod_id"], e["pid"], e["conn_h"] = ts, trace, pod, pid, conn
        e["svc_id"], e["node_id"] = svc, node
        if typ is None:
            typ = self.rng.choice(_TYPES, n)
            if mix42:
                typ = np.where(self.rng.random(n) < 0.03, np.uint16(UNSUPPORTED_TYPE), typ)
        e["signal_type"] = typ
        e["tid"] = e["pid"]
        scale = np.array([_SCALE.get(int(t), 1.0) for t in e["signal_type"]])
        raw = np.where(scale == 1e-6, self.rng.integers(100_000, 400_000_000, n),
                       np.where(scale == 1.0, self.rng.integers(0, 12, n), self.rng.integers(0, 100_000, n)))
        e["value"] = raw.astype(np.uint64)
        self.ev.append(e)
        idx = np.arange(self.n_ev, self.n_ev + n)
        self.n_ev += n
        return idx

    def spans(self, ts, trace=0, pod=0, pid=0, conn=0, svc=0, node=0, group=0) -> np.ndarray:
        ts = np.atleast_1d(np.asarray(ts, dtype=np.int64))
        n = len(ts)
        s = np.zeros(n, dtype=records.SPAN)
        s["ts_ns"], s["trace_h"], s["pod_id"], s["pid"], s["conn_h"] = ts, trace, pod, pid, conn
        s["svc_id"], s["node_id"], s["group_id"] = svc, node, group
        s["ttft_ms"] = self.rng.uniform(50.0, 1500.0, n).astype(np.float32)
        s["latency_ms"] = s["ttft_ms"] * np.float32(2.0)
        s["span_h"] = self.rng.integers(1, 1 << 62, n).astype(np.uint64)
        self.sp.append(s)
        idx = np.arange(self.n_sp, self.n_sp + n)
        self.n_sp += n
        return idx

    def build(self, name: str, n_groups: int, params, info: dict = None) -> JoinCase:
        ev = np.concatenate(self.ev) if self.ev else np.zeros(0, dtype=records.EVENT)
        sp = np.concatenate(self.sp) if self.sp else np.zeros(0, dtype=records.SPAN)
        assert len(ev) <= MAX_EVENTS and len(sp) <= MAX_SPANS, (name, len(ev), len(sp))
        pe, ps = self.rng.permutation(len(ev)), self.rng.permutation(len(sp))
        pos_e, pos_s = np.empty(len(ev), np.int64), np.empty(len(sp), np.int64)
        pos_e[pe], pos_s[ps] = np.arange(len(ev)), np.arange(len(sp))  # pre-shuffle index -> input row
        ev, sp = ev[pe].copy(), sp[ps].copy()
        ev.setflags(write=False)
        sp.setflags(write=False)

        def remap(v, pos):
            if isinstance(v, dict):
                return {k: remap(x, pos) for k, x in v.items()}
            return pos[np.asarray(v, dtype=np.int64)]

        out = {}
        for key, v in (info or {}).items():
            if key.startswith("ev_"):
                out[key] = remap(v, pos_e)
            elif key.startswith("sp_"):
                out[key] = remap(v, pos_s)
            else:
                out[key] = v
        return JoinCase(name, ev, sp, n_groups, tuple(params), out)


def _id(n: int) -> int:
    """A fixed, well-mixed 64-bit identity (trace / connection hashes)."""
    return records.splitmix64(0xC0FFEE00 + n) | 1


# ---- the cases -------------------------------------------------------------------------------

def _boundaries() -> JoinCase:
    w = _Window(101)
    T = [EPOCH_NS + i * 10_000 * MS for i in range(4)]
    # the span of tier k and the identity its signals share with it: that tier's key only
    span_id = [dict(trace=_id(10 + k), pod=10 + k, pid=100 + k, conn=_id(20 + k), svc=3 + k, node=40 + k) for k in range(4)]
    other = dict(trace=_id(30), pod=90, pid=900, conn=_id(31), svc=60, node=61)
    share = (("trace",), ("pod", "pid"), ("pod", "conn"), ("svc", "node"))
    sp_idx, at, past, inside = {}, {}, {}, {}
    for k in range(4):
        sp_idx[k] = w.spans(T[k], group=k, **span_id[k])
        sig_id = dict(other, **{f: span_id[k][f] for f in share[k]})
        at[k], past[k], inside[k] = {}, {}, {}
        for win in TIER_WINDOWS_MS:
            d = win * MS
            typ = _TYPES[(k + win) % len(_TYPES)]
            at[k][win] = w.signals([T[k] + d, T[k] - d], typ=typ, **sig_id)
            inside[k][win] = w.signals([T[k] + d - 1, T[k] - d + 1], typ=typ, **sig_id)
            past[k][win] = w.signals([T[k] + d + 1, T[k] - d - 1], typ=typ, **sig_id)
        w.signals([T[k] + 5 * MS], typ=UNSUPPORTED_TYPE, **sig_id)
    params = [_params(window_ms=ms, threshold=thr) for ms in (2000, 100, 300) for thr in (0.7, 0.6)]
    return w.build("boundaries", 4, params, dict(sp_tier=sp_idx, ev_at=at, ev_past=past, ev_inside=inside))


def _boundaries_wide() -> JoinCase:
    w = _Window(102)
    T = EPOCH_NS + 40_000 * MS
    a = dict(trace=_id(40), pod=41, pid=410, conn=_id(41), svc=4, node=41)
    b = dict(trace=_id(42), pod=42, pid=420, conn=_id(43), svc=4, node=42)
    far = 33_900 * MS
    w.spans(T, group=0, **a)
    w.spans(T + 7 * MS, group=1, **b)
    for d in (far, 34_000 * MS - 1, 34_000 * MS, 34_000 * MS + 1):
        w.signals([T + d, T - d], trace=a["trace"], pod=99, pid=990, conn=_id(44), svc=9, node=9)
    # span b: two trace pairs at 33.9 s, then pod-tier pairs right behind them in the top-3
    w.signals([T + 7 * MS + far, T + 7 * MS - far], trace=b["trace"], pod=99, pid=990, conn=_id(44), svc=9, node=9)
    w.signals([T + 57 * MS, T - 43 * MS], trace=_id(45), pod=b["pod"], pid=b["pid"], conn=_id(44), svc=9, node=9)
    w.signals([T + 207 * MS], trace=_id(45), pod=b["pod"], pid=991, conn=b["conn"], svc=9, node=9)
    w.signals([T + far, T + 3 * MS], typ=UNSUPPORTED_TYPE, **a)
    return w.build("boundaries_wide", 2, [_params(window_ms=34000), _params(window_ms=34000, threshold=0.6, group_mode=0)])


def _zero_keys() -> JoinCase:
    w = _Window(103)
    T = EPOCH_NS + 80_000 * MS
    fields = ("trace", "pod", "pid", "conn", "svc", "node")
    a = dict(trace=_id(50), pod=50, pid=500, conn=_id(51), svc=5, node=50)
    b = dict(trace=_id(52), pod=52, pid=520, conn=_id(53), svc=6, node=52)  # differs from a in every field
    ev_b = []
    for mask in range(128):
        zeroed = {f: 0 for i, f in enumerate(fields) if mask >> i & 1}
        ts_zero = bool(mask >> 6 & 1)
        w.spans(0 if ts_zero else T + (mask % 5) * MS, group=mask % 4, **dict(a, **zeroed))
        w.signals([0 if ts_zero else T + 10 * MS], **dict(a, **zeroed))
        ev_b.append(w.signals([0 if ts_zero else T + 20 * MS], **dict(b, **zeroed)))
    w.signals([T + 1 * MS, T + 2 * MS], typ=UNSUPPORTED_TYPE, **a)
    w.signals([0, 0, 0])  # all-zero records
    return w.build("zero_keys", 4, [_params(), _params(threshold=0.6, group_mode=0)],
                   dict(ev_other_identity=np.concatenate(ev_b)))


def _precedence() -> JoinCase:
    w = _Window(104)
    T = EPOCH_NS + 120_000 * MS
    a = dict(trace=_id(60), pod=60, pid=600, conn=_id(61), svc=7, node=60)
    x = dict(trace=_id(62), pid=601, conn=_id(63), svc=8, node=61)  # the unequal values
    w.spans(T, group=0, **a)
    w.spans(T + 30 * MS, group=1, **a)
    n = 0
    for tr_eq, pid_eq, cn_eq, sn_eq in itertools.product((True, False), repeat=4):
        ident = dict(pod=a["pod"], trace=a["trace"] if tr_eq else x["trace"], pid=a["pid"] if pid_eq else x["pid"],
                     conn=a["conn"] if cn_eq else x["conn"], svc=a["svc"] if sn_eq else x["svc"],
                     node=a["node"] if sn_eq else x["node"])
        for dt in (50, 200, 400, 1500):
            w.signals([T + dt * MS, T - dt * MS], typ=_TYPES[n % 5], **ident)
            n += 1
    w.signals([T + 50 * MS, T - 200 * MS, T + 400 * MS, T - 1500 * MS], typ=UNSUPPORTED_TYPE, **a)
    params = [_params(threshold=thr, fanout=fo, group_mode=gm) for thr in (0.6, 0.7, 0.85, 0.95, 1.5)
              for fo in (1, 2, 3) for gm in (1, 0)]
    return w.build("precedence", 2, params)


def _ranking() -> JoinCase:
    w = _Window(105)
    T = EPOCH_NS + 160_000 * MS
    shared = dict(pod=70, pid=700, conn=_id(70), svc=9, node=70)
    away = dict(pod=79, pid=790, conn=_id(79), svc=19, node=79)
    three = _TYPES[:3]  # few slots: matched signals share slots, the max-merge picks a value
    tr_dts = (70, -70, 70, 300, -900, 1200, -5)  # ms: a +-70 tie, a duplicate timestamp
    n_tr = (0, 1, 2, 3, 5, 0, 1, 2, 3, 6, 4, 2)
    for i, k in enumerate(n_tr):
        t = T + i * 3000 * MS
        trace = _id(100 + i)
        w.spans(t, trace=trace, group=i % 3, **shared)
        if i in (4, 8):  # a second span of the same request, 40 ms later
            w.spans(t + 40 * MS, trace=trace, group=(i + 1) % 3, **shared)
        for j, dt in enumerate(tr_dts[:k]):  # every other trace signal is the span's own process as well
            ident = shared if j % 2 else away
            w.signals([t + dt * MS], trace=trace, typ=three[j % 3], **ident)
        w.signals(t + np.array([20, -20, 20, -60, 99]) * MS, typ=three[i % 3], **dict(away, pod=70, pid=700))
        w.signals(t + np.array([150, -150, 150, 240]) * MS, typ=three[(i + 1) % 3], **dict(away, pod=70, conn=shared["conn"]))
        w.signals(t + np.array([300, -300]) * MS, typ=three[(i + 2) % 3], **dict(away, svc=9, node=70))
        w.signals([t + 1 * MS], trace=trace, typ=UNSUPPORTED_TYPE, **shared)
    for i, k in enumerate((0, 1, 2, 3)):  # spans that only a trace id can match
        t = T + (40 + i) * 3000 * MS
        trace = _id(140 + i)
        w.spans(t, trace=trace, group=i % 3)
        w.signals(t + np.array([25, -25, 25][:k], dtype=np.int64) * MS, trace=trace, typ=three[0], **away)
    params = [_params(), _params(group_mode=0), _params(threshold=0.6), _params(threshold=0.85, fanout=2),
              _params(threshold=0.95, fanout=1, group_mode=0)]
    return w.build("ranking", 3, params)


def _mixed_runs() -> JoinCase:
    w = _Window(106)
    T = EPOCH_NS + 400_000 * MS
    dts = np.arange(-320, 321, 20) * MS
    # (a) one (pod, pid), spans differ in group, svc|node and conn
    ca = (_id(200), _id(201), 0)
    for i, off in enumerate((0, 10, 10, 35, 60, 90, 120, 200)):
        w.spans(T + off * MS, trace=_id(210) if i % 4 == 0 else 0, pod=30, pid=300, conn=ca[i % 3], svc=7,
                node=8 + i % 2, group=i % 3)
    for j, dt in enumerate(dts):
        w.signals([T + dt + j], trace=_id(210) if j % 5 == 0 else _id(211), pod=30, pid=300,
                  conn=(ca[0], ca[1], _id(202))[j % 3], svc=(7, 7, 1)[j % 3], node=(8, 9, 1)[(j // 3) % 3])
    # (b) one (pod, conn), spans differ in pid: some the signals' pid, some not, one none
    Tb, cb = T + 5000 * MS, _id(220)
    for i, off in enumerate((0, 15, 15, 50, 80, 130, 180, 260)):
        w.spans(Tb + off * MS, trace=_id(230 + i), pod=31, pid=(310, 311, 312, 0)[i % 4], conn=cb, svc=7, node=31, group=1)
    for j, dt in enumerate(dts):
        w.signals([Tb + dt, Tb + dt + 7 * MS], pod=31, pid=(310, 999)[j % 2], conn=cb, svc=(7, 2)[j % 2], node=31)
    # (b') a uniform (pod, conn) run whose pid the signals share or not: the P2 sub-range in range accounting
    Tc, cc = T + 10_000 * MS, _id(240)
    w.spans(Tc + np.array([0, 40, 40, 110, 190, 280]) * MS, pod=32, pid=320, conn=cc, svc=7, node=32, group=2)
    for j, dt in enumerate(dts):
        w.signals([Tc + dt], pod=32, pid=(320, 998, 320)[j % 3], conn=(cc, cc, _id(241))[j % 3], svc=7, node=(32, 33)[j % 2])
    # (c) constructed pod+conn hash collisions: the span list holds key A only / both keys
    Td, cd = T + 15_000 * MS, _id(250)
    cd2 = colliding_conn(33, cd, 34)
    w.spans(Td + np.array([0, 30, 30, 90, 170]) * MS, pod=33, pid=330, conn=cd, svc=7, node=33, group=0)
    for j, dt in enumerate(dts):
        w.signals([Td + dt], pod=(34, 33)[j % 2], pid=(340, 331)[j % 2], conn=(cd2, cd)[j % 2], svc=2, node=33)
    Te, ce = T + 20_000 * MS, _id(260)
    ce2 = colliding_conn(35, ce, 36)
    for i, off in enumerate((0, 20, 20, 70, 140, 210)):
        w.spans(Te + off * MS, pod=(35, 36)[i % 2], pid=350, conn=(ce, ce2)[i % 2], svc=7, node=35, group=i % 3)
    for j, dt in enumerate(dts):
        w.signals([Te + dt], pod=(35, 36)[j % 2], pid=(351, 350)[(j // 2) % 2], conn=(ce, ce2)[j % 2], svc=2, node=35)
    w.signals(T + np.arange(8) * 11 * MS, typ=UNSUPPORTED_TYPE, pod=30, pid=300, conn=ca[0], svc=7, node=8)
    params = [_params(), _params(group_mode=0), _params(threshold=0.6), _params(threshold=0.85),
              _params(threshold=0.95, fanout=2), _params(window_ms=150)]
    return w.build("mixed_runs", 3, params,
                   dict(collisions=(((33, cd), (34, cd2)), ((35, ce), (36, ce2)))))


def _long_lists() -> JoinCase:
    w = _Window(107)
    rng = w.rng
    T = EPOCH_NS + 600_000 * MS
    ident = dict(pod=80, pid=800, conn=_id(300), svc=10, node=80)
    span_ms = 5000
    # 600 spans on one key, 25 ms grid with duplicates, 3 groups; 300 share 4 trace ids, 100 have none
    ts = T + rng.integers(0, span_ms // 25, 600) * 25 * MS
    shared_tr = np.array([_id(310 + i) for i in range(4)], dtype=np.uint64)
    trace = np.array([_id(1000 + i) for i in range(600)], dtype=np.uint64)
    trace[:300] = shared_tr[rng.integers(0, 4, 300)]
    trace[300:400] = 0
    w.spans(ts, trace=trace, group=rng.integers(0, 3, 600), **ident)
    n = 6900
    sts = T + rng.integers(-300 * MS, (span_ms + 300) * MS, n)
    on_grid = rng.random(n) < 0.2  # exact |dt| ties with spans of the grid
    sts = np.where(on_grid, T + rng.integers(0, span_ms // 25, n) * 25 * MS, sts)
    pid = np.where(rng.random(n) < 0.7, 800, 801)
    conn = np.where(rng.random(n) < 0.5, np.uint64(ident["conn"]), np.uint64(_id(301)))
    u = rng.random(n)
    strace = np.where(u < 0.08, shared_tr[rng.integers(0, 4, n)],
                      np.where(u < 0.12, trace[rng.integers(400, 600, n)], np.uint64(0)))
    node = np.where(rng.random(n) < 0.9, 80, 81)
    w.signals(sts, trace=strace, pod=80, pid=pid, conn=conn, svc=10, node=node, mix42=True)
    # a second list: 300 spans on one uniform key (one group): range accounting over chunks 256 + 44
    ts2 = T + rng.integers(0, 3000 // 25, 300) * 25 * MS
    w.spans(ts2, pod=81, pid=810, conn=_id(302), svc=11, node=81, group=2)
    m = 1200
    sts2 = T + rng.integers(-300 * MS, 3300 * MS, m)
    w.signals(sts2, pod=81, pid=np.where(rng.random(m) < 0.6, 810, 811),
              conn=np.where(rng.random(m) < 0.6, np.uint64(_id(302)), np.uint64(_id(303))), svc=11, node=81, mix42=True)
    params = [_params(), _params(group_mode=0), _params(threshold=0.6), _params(threshold=0.85, fanout=2)]
    return w.build("long_lists", 3, params)


def _sliced_lists() -> JoinCase:
    w = _Window(108)
    rng = w.rng
    T = EPOCH_NS + 700_000 * MS
    X = _id(400)
    span_ms = 3000
    # 32 spans on the big key (one group: a uniform run), 8 of the same pod under another pid
    ts = T + rng.integers(0, span_ms, 40) * MS
    trace = np.where(np.arange(40) % 4 == 0, np.uint64(X), np.array([_id(410 + i) for i in range(40)], dtype=np.uint64))
    pid = np.where(np.arange(40) < 32, 900, 901)
    group = np.where(np.arange(40) < 32, 0, 1 + np.arange(40) % 2)
    w.spans(ts, trace=trace, pod=90, pid=pid, conn=_id(401), svc=12, node=90, group=group)
    n = 6400  # one (pod, pid), one trace id, one svc|node: three lists longer than a work item
    sts = T + rng.integers(-200 * MS, (span_ms + 200) * MS, n)
    w.signals(sts, trace=X, pod=90, pid=900, conn=np.where(rng.random(n) < 0.3, np.uint64(_id(401)), np.uint64(_id(402))),
              svc=12, node=90)
    m = 1700
    sts = T + rng.integers(-200 * MS, (span_ms + 200) * MS, m)
    w.signals(sts, trace=np.where(rng.random(m) < 0.3, np.uint64(X), np.uint64(0)), pod=90,
              pid=np.where(rng.random(m) < 0.5, 901, 902), conn=_id(401), svc=12, node=np.where(rng.random(m) < 0.5, 90, 91),
              mix42=True)
    params = [_params(), _params(group_mode=0), _params(threshold=0.6, fanout=2)]
    return w.build("sliced_lists", 3, params,
                   dict(big_keys=dict(trace=X, pod=90, pid=900, svcnode=(12 << 16) | 90)))


def _many_groups(n_groups: int) -> JoinCase:
    w = _Window(109 + n_groups)
    rng = w.rng
    T = EPOCH_NS + 800_000 * MS
    S, N = 240, 2400
    pods = 60 + rng.integers(0, 6, S)
    group = rng.integers(0, n_groups + 12, S).astype(np.uint32)  # some at and beyond n_groups: ignored
    group[:4] = (n_groups - 1, n_groups, 0xFFFFFFFF, 1 << 31)
    strace = np.array([_id(2000 + i) for i in range(S)], dtype=np.uint64)
    w.spans(T + rng.integers(0, 2000, S) * MS, trace=strace, pod=pods, pid=pods * 10, conn=_id(500), svc=13,
            node=pods, group=group)
    epod = 60 + rng.integers(0, 6, N)
    w.signals(T + rng.integers(-100 * MS, 2100 * MS, N), trace=np.where(rng.random(N) < 0.3, strace[rng.integers(0, S, N)], np.uint64(0)),
              pod=epod, pid=np.where(rng.random(N) < 0.6, epod * 10, 7), conn=np.where(rng.random(N) < 0.5, np.uint64(_id(500)), np.uint64(0)),
              svc=13, node=epod, mix42=True)
    params = [_params(), _params(group_mode=0), _params(threshold=0.6)]
    return w.build(f"many_groups_{n_groups}", n_groups, params)


HALO_MS = 2000.0


@functools.lru_cache(maxsize=None)
def halo_pair() -> Tuple[JoinCase, JoinCase]:
    """Two consecutive windows for an engine with a halo of ``HALO_MS``: the second window's spans
    match first-window rows that stay visible (ts >= the first window's latest record - halo), some
    exactly at that cut-off and some 1 ns before it (hidden), and some of the visible matches tie in
    |dt| with rows of the second window (this window's rows come first in the join's row order)."""
    T1 = EPOCH_NS + 1_000_000 * MS  # the first window's latest record
    cut = T1 - int(HALO_MS) * MS
    a = dict(trace=_id(600), pod=95, pid=950, conn=_id(601), svc=14, node=95)
    b = dict(trace=_id(602), pod=96, pid=960, conn=_id(603), svc=14, node=96)
    none = dict(pod=0, pid=0, conn=0, svc=0, node=0)
    params = [_params(), _params(group_mode=0, fanout=2)]
    w1 = _Window(121)
    w1.signals([T1], typ=1, pod=97, pid=970, svc=15, node=97)
    late = T1 - 500 * MS  # a span of the second window that started before the first one ended
    at_cut = w1.signals([cut, cut, cut + 1], typ=1, trace=a["trace"], **none)
    hidden = w1.signals([cut - 1, cut - 1, cut - 2 * MS], typ=1, trace=a["trace"], **none)
    w1.signals(late + np.array([-40, 25, -300]) * MS, trace=a["trace"], **none)
    # identity b around the cut between the windows: ties at +-10, +-60 ms of the second window's span
    Tb = T1 + 10 * MS
    w1.signals(Tb - np.array([20, 20, 60, 95]) * MS, pod=b["pod"], pid=b["pid"], conn=_id(604), svc=1, node=1)
    w1.signals(Tb - np.array([150, 240]) * MS, pod=b["pod"], pid=961, conn=b["conn"], svc=1, node=1)
    w1.signals(Tb - np.array([30, 30, 700]) * MS, typ=3, trace=b["trace"], **none)
    w1.signals(T1 - w1.rng.integers(0, 1900, 200) * MS, pod=95, pid=np.where(w1.rng.random(200) < 0.5, 950, 951),
               conn=a["conn"], svc=14, node=95, mix42=True)
    w1.spans(T1 - np.array([100, 400, 900, 1300]) * MS, trace=_id(610), group=np.arange(4) % 3, **{k: v for k, v in a.items() if k != "trace"})
    first = w1.build("halo_first", 3, params, dict(ev_at_cut=at_cut, ev_hidden=hidden))
    w2 = _Window(122)
    w2.signals([T1 + 1500 * MS], typ=1, pod=97, pid=970, svc=15, node=97)
    w2.spans([late], trace=a["trace"], group=0, **none)
    w2.spans([late + 5 * MS], group=1, **a)
    w2.signals(late + np.array([40, -25]) * MS, trace=a["trace"], **none)  # |dt| ties with first-window rows (late records)
    w2.spans([Tb, Tb + 3 * MS], group=[1, 2], **b)
    w2.signals(Tb + np.array([20, 60, 95, 99]) * MS, pod=b["pod"], pid=b["pid"], conn=_id(604), svc=1, node=1)
    w2.signals(Tb + np.array([150, 240]) * MS, pod=b["pod"], pid=961, conn=b["conn"], svc=1, node=1)
    w2.signals(Tb + np.array([30, 700]) * MS, typ=3, trace=b["trace"], **none)
    w2.signals(T1 + w2.rng.integers(1, 1400, 200) * MS, pod=95, pid=np.where(w2.rng.random(200) < 0.5, 950, 951),
               conn=a["conn"], svc=14, node=95, mix42=True)
    w2.spans(T1 + np.array([50, 60, 400, 900]) * MS, trace=_id(611), group=np.arange(4) % 3, **{k: v for k, v in a.items() if k != "trace"})
    second = w2.build("halo_second", 3, params)
    return first, second


@functools.lru_cache(maxsize=None)
def cases() -> Dict[str, JoinCase]:
    """Every named case (built once per process; the record arrays are read-only)."""
    built = [_boundaries(), _boundaries_wide(), _zero_keys(), _precedence(), _ranking(), _mixed_runs(),
             _long_lists(), _sliced_lists(), _many_groups(65), _many_groups(100)]
    return {c.name: c for c in built}
