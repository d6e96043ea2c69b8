"""Copy ahead (ops/csrc/engine.hip ``submit_copy`` / ``submit_chain``, pipeline/window.py
``stage_copy`` / ``stage_chain``, agent/worker.py ``WorkerCore.window``): window k's DMAs are issued
before window k - nb's results are collected, behind a host wait for that window's front stage.

Engine level, for 2, 3 and 4 buffers: 4 nb + 1 seeded replay windows of differing sizes -- among
them an empty one, one whose kernel range arrives as two segments with a record split between them
(a range that wraps the ring) and one from memory that is not page-locked (pinned staging) -- go
through ``submit`` back to back, through the two phases with window k - nb's packet and results
read between them (two lanes, and one lane), and through an engine that waits after every window.
Every window's packet and result block is byte-identical in the four runs; the timing events of
every uncollected window answer for that window (finite, non-negative); copies are reported in
window order. Worker level: one cut sequence through ``WorkerCore.window`` with copy-ahead on and
with MISLO_COPY_AHEAD=0 returns the same windows in the same order with the same bytes, and the
configurations that keep the plain order say so through ``copy_ahead``. Three buffers start on
one copy lane; the caller that copies ahead takes the second (``take_copy_lanes``), also in the
middle of a run."""

import dataclasses
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIG_CAP, SPAN_CAP, GROUPS, USER_CAP = 4096, 256, 8, 2048
HALO_MS = 2000.0  # windows are 1 s apart: with the current one, three generations are resident
REC = 136         # a framed batch record (collector/records.py REC_STRIDE)


def _images(n):
    """n replay windows of differing sizes (seeded); window 3 is empty."""
    from llm_slo_ebpf_toolkit_amd.pipeline.replay import ReplayConfig, ReplayGenerator
    from llm_slo_ebpf_toolkit_amd.pipeline.window import build_replay_images

    cfg = ReplayConfig(scenario="full", n_nodes=2, pods_per_node=8, n_services=GROUPS, events_per_window=2048,
                       spans_per_window=SPAN_CAP, seed=61)
    gen = ReplayGenerator(cfg)
    rng = np.random.default_rng(61)
    wins = []
    for j in range(n):
        w = gen.next_window()
        ne = 0 if j == 3 else int(rng.integers(64, len(w.events) + 1))
        ns = 0 if j == 3 else int(rng.integers(8, min(len(w.spans), SPAN_CAP) + 1))
        wins.append(dataclasses.replace(w, events=np.ascontiguousarray(w.events[:ne]),
                                        spans=np.ascontiguousarray(w.spans[:ns])))
    sn = (gen.pod_svc.astype(np.uint32) << np.uint32(16)) | gen.pod_node.astype(np.uint32)
    return build_replay_images(wins), (gen.pod_ids.astype(np.uint32), sn)


@pytest.fixture(scope="module")
def replay():
    """17 windows (4 x 4 buffers + 1) and the pod table, built once and never changed; runs with
    fewer buffers take a prefix."""
    return _images(17)


class _Arena:
    """Host memory the windows' segments point into: one page-locked block holding every window's
    bytes at its own offset (a window's bytes stay untouched for the whole run), and a block that
    is never page-locked for the window that goes through pinned staging."""

    def __init__(self, eng, imgs, wrap, unregistered):
        blobs = [(np.ascontiguousarray(i.framed).view(np.uint8).reshape(-1),
                  np.ascontiguousarray(i.user).view(np.uint8).reshape(-1),
                  np.ascontiguousarray(i.spans).view(np.uint8).reshape(-1)) for i in imgs]
        total = sum(len(b) + 64 for t in blobs for b in t) + 4096
        self.pinned = np.zeros(total, dtype=np.uint8)
        self.loose = np.zeros(sum(len(b) + 64 for b in blobs[unregistered]) + 64, dtype=np.uint8)
        assert eng.register_host(self.pinned.ctypes.data, self.pinned.nbytes)
        self.segs = []
        off = {id(self.pinned): 0, id(self.loose): 0}

        def put(block, b):
            o = off[id(block)]
            block[o:o + len(b)] = b
            off[id(block)] = o + ((len(b) + 63) & ~63)
            return (block.ctypes.data + o, len(b))

        for j, (fr, us, sp) in enumerate(blobs):
            block = self.loose if j == unregistered else self.pinned
            if j == wrap:  # as a range that wraps the ring: its tail first, cut inside a record
                cut = REC * (len(fr) // REC // 2) + 52
                assert 0 < cut < len(fr)
                second = put(block, fr[cut:])
                kern = [put(block, fr[:cut]), second]
            else:
                kern = [put(block, fr)] if len(fr) else []
            self.segs.append((kern, [put(block, us)] if len(us) else [], [put(block, sp)] if len(sp) else []))


def _engine(monkeypatch, nb, lanes, ahead, default_lanes=False):
    """``default_lanes``: MISLO_COPY_LANES unset (``lanes`` = what the engine then starts with)."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    if default_lanes:
        monkeypatch.delenv("MISLO_COPY_LANES", raising=False)
    else:
        monkeypatch.setenv("MISLO_COPY_LANES", str(lanes))
    monkeypatch.setenv("MISLO_COPY_AHEAD", "1" if ahead else "0")
    pipe = WindowPipeline(SIG_CAP, SPAN_CAP, GROUPS, model="bayes", learn=False, user_cap=USER_CAP, halo_ms=HALO_MS,
                          n_buffers=nb, max_ahead=nb)
    assert pipe.eng.copy_lanes == lanes and pipe.eng.copy_ahead == ahead and pipe.eng.buffers == nb
    return pipe


def _read(eng, k, n_groups):
    eng.wait(k)
    res = eng.results(k, n_groups)
    return np.array(eng.packet(k), copy=True), {key: np.array(res[key], copy=True) for key in res}


def _check_times(eng, k, one_lane):
    """Window k's own timing records: they end in the past and follow each other."""
    total, comp = eng.window_ms(k)
    dur, gap = eng.copy_ms(k)
    for v in (total, comp, dur, gap):
        assert math.isfinite(v), (k, total, comp, dur, gap)
    assert total >= 0 and comp >= 0 and dur >= 0 and total >= dur, (k, total, comp, dur)
    if one_lane and k >= 1:  # one in-order copy stream: window k's first DMA follows window k - 1's last
        assert gap >= 0, (k, gap)


def _run(monkeypatch, replay, nb, mode, lanes=1):
    """4 nb + 1 windows through one engine. ``mode``: "wait" (submit, then wait for the window),
    "submit" (back to back: window k - nb is read just before submit(k) overwrites it) or "phases"
    (copy phase, read window k - nb, chain phase)."""
    imgs, pods = replay
    n = 4 * nb + 1
    imgs = imgs[:n]
    wrap, unregistered = 5, 6
    pipe = _engine(monkeypatch, nb, lanes, ahead=mode == "phases")
    eng = pipe.eng
    eng.set_pods(*pods)
    arena = _Arena(eng, imgs, wrap, unregistered)
    assert len(arena.segs[wrap][0]) == 2 and not any(arena.segs[3])  # two segments; the empty window
    out = {}
    for k, img in enumerate(imgs):
        kern, user, spans = arena.segs[k]
        args = (k, kern, user, spans, img.n_groups, img.labels, [int(b) for b in img.bases])
        if mode == "phases":
            assert not eng.h2d_done(k)
            eng.submit_copy(*args, 64)
            assert not eng.h2d_done(k + 1)
            if eng.h2d_done(k):  # every window up to k: wait_h2d(k) returns, the earlier ones say so too
                assert all(eng.h2d_done(j) for j in range(k))
            if k % 3 == 0:
                eng.wait_h2d(k)
                assert eng.h2d_done(k) and (k == 0 or eng.h2d_done(k - 1))
            if k >= nb:  # its copy-side events were recorded for window k a moment ago
                if k == 2 * nb:  # every uncollected window, once (this waits for them all)
                    for j in range(k - nb, k):
                        _check_times(eng, j, lanes == 1)
                _check_times(eng, k - nb, lanes == 1)
                out[k - nb] = _read(eng, k - nb, imgs[k - nb].n_groups)
            eng.submit_chain(k, img.n_groups, True, False)
        else:
            if mode == "submit" and k >= nb:
                out[k - nb] = _read(eng, k - nb, imgs[k - nb].n_groups)
            eng.submit(*args, True, False, 64)
            if mode == "wait":
                out[k] = _read(eng, k, img.n_groups)
    for k in range(max(0, n - nb), n):
        if k not in out:
            _check_times(eng, k, lanes == 1)
            out[k] = _read(eng, k, imgs[k].n_groups)
    eng.wait_h2d(n - 1)
    assert all(eng.h2d_done(k) for k in range(n)) and not eng.h2d_done(n)
    staged = sum(nbytes for part in arena.segs[unregistered] for _, nbytes in part)
    assert int(eng.staged_bytes) == staged > 0
    pipe.drain()
    pipe.close()
    return [out[k] for k in range(n)]


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for k in range(len(a)):
        assert a[k][0].tobytes() == b[k][0].tobytes(), f"{what}: packet of window {k}"
        assert sorted(a[k][1]) == sorted(b[k][1])
        for key in a[k][1]:
            assert a[k][1][key].tobytes() == b[k][1][key].tobytes(), f"{what}: {key} of window {k}"


@pytest.mark.parametrize("nb", [2, 3, 4])
def test_phases_compute_what_submit_computes(monkeypatch, replay, nb):
    waited = _run(monkeypatch, replay, nb, "wait")
    assert any(pk.any() for pk, _ in waited)
    _assert_same(_run(monkeypatch, replay, nb, "submit"), waited, "submit back to back against waiting")
    _assert_same(_run(monkeypatch, replay, nb, "phases", lanes=2), waited, "two phases, two lanes")
    _assert_same(_run(monkeypatch, replay, nb, "phases", lanes=1), waited, "two phases, one lane")


def test_phases_are_refused_out_of_order(monkeypatch, replay):
    imgs, pods = replay
    pipe = _engine(monkeypatch, 3, 1, True)
    eng = pipe.eng
    arena = _Arena(eng, imgs[:2], wrap=-1, unregistered=1)
    img = imgs[0]
    with pytest.raises(Exception):
        eng.submit_chain(0, img.n_groups, True, False)
    eng.submit_copy(0, *arena.segs[0], img.n_groups, img.labels, [int(b) for b in img.bases], 64)
    with pytest.raises(Exception):
        eng.submit_copy(0, *arena.segs[0], img.n_groups, img.labels, [int(b) for b in img.bases], 64)
    with pytest.raises(Exception):
        eng.submit_chain(0, img.n_groups - 1, True, False)
    eng.submit_chain(0, img.n_groups, True, False)
    eng.wait(0)
    pipe.close()


def test_defaults_and_the_lane_taken_on_request(monkeypatch, replay):
    """Without the switches: copy-ahead wherever windows overlap; two lanes from four buffers on;
    three buffers start on one lane and run two once the caller that copies ahead has asked
    (``take_copy_lanes``), here in the middle of a run; two buffers, and engines without
    copy-ahead, keep what they have."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    imgs, pods = replay
    waited = _run(monkeypatch, replay, 3, "wait")
    for name in ("MISLO_COPY_LANES", "MISLO_COPY_AHEAD", "MISLO_WINDOW_OVERLAP"):
        monkeypatch.delenv(name, raising=False)

    def pipeline(nb):
        return WindowPipeline(SIG_CAP, SPAN_CAP, GROUPS, model="bayes", learn=False, user_cap=USER_CAP,
                              halo_ms=HALO_MS, n_buffers=nb, max_ahead=nb)

    def lanes(nb):  # (copy-ahead, lanes at construction, lanes once asked for)
        pipe = pipeline(nb)
        got = (bool(pipe.eng.copy_ahead), int(pipe.eng.copy_lanes), pipe.prepare_copy_ahead(),
               int(pipe.eng.copy_lanes))
        pipe.close()
        return got

    assert [lanes(nb) for nb in (2, 3, 4)] == [(True, 1, True, 1), (True, 1, True, 2), (True, 2, True, 2)]
    monkeypatch.setenv("MISLO_COPY_LANES", "1")
    assert lanes(3) == (True, 1, True, 1)
    monkeypatch.delenv("MISLO_COPY_LANES")
    monkeypatch.setenv("MISLO_COPY_AHEAD", "0")
    assert [lanes(nb) for nb in (3, 4)] == [(False, 1, False, 1), (False, 2, False, 2)]
    monkeypatch.delenv("MISLO_COPY_AHEAD")
    # windows 0 and 1 by submit on one lane, still in flight when the lane is taken; the rest in phases
    pipe = pipeline(3)
    eng = pipe.eng
    eng.set_pods(*pods)
    arena = _Arena(eng, imgs[:9], wrap=5, unregistered=6)
    out = {}
    for k, img in enumerate(imgs[:9]):
        args = (k, *arena.segs[k], img.n_groups, img.labels, [int(b) for b in img.bases])
        if k < 2:
            eng.submit(*args, True, False, 64)
            assert eng.copy_lanes == 1
            continue
        if k == 2:
            assert eng.take_copy_lanes() and eng.copy_lanes == 2
        eng.submit_copy(*args, 64)
        if k >= 3:
            _check_times(eng, k - 3, False)
            out[k - 3] = _read(eng, k - 3, imgs[k - 3].n_groups)
        eng.submit_chain(k, img.n_groups, True, False)
    for k in range(6, 9):
        out[k] = _read(eng, k, imgs[k].n_groups)
    eng.wait_h2d(8)
    assert all(eng.h2d_done(k) for k in range(9))
    _assert_same([out[k] for k in range(9)], waited[:9], "the second lane taken at window 2")
    pipe.close()


# ---- worker level -------------------------------------------------------------------------------

def _rings(tag):
    from llm_slo_ebpf_toolkit_amd.runtime import load

    rt = load()
    return (rt.Ringbuf.create_shm(f"/mislo-ca-{os.getpid()}-{tag}", 1 << 22), rt.HostRing(1 << 14, 64),
            rt.HostRing(1 << 12, 64))


def _worker_run(monkeypatch, replay, ahead, tag):
    from llm_slo_ebpf_toolkit_amd.agent.worker import WorkerCore, WorkerSpec
    from llm_slo_ebpf_toolkit_amd.pipeline.window import Cut, RingWindowSource

    imgs, pods = replay
    imgs = imgs[:13]
    pipe = _engine(monkeypatch, 3, 1, ahead, default_lanes=True)
    assert pipe.copy_ahead == ahead
    rb, user, spans = _rings(tag)
    src = RingWindowSource(pipe, rb, user, spans)
    pipe.eng.set_pods(*pods)
    spec = WorkerSpec(rank=0, world=1, device=0, engine="gpu", source="shm", ring_name=tag, pin_dir="", user_rec=64,
                      sig_cap=SIG_CAP, span_cap=SPAN_CAP, group_cap=GROUPS, user_cap=USER_CAP, window_ms=1000.0,
                      ttft_slo_ms=800.0, halo_ms=HALO_MS, import_cap=0, xchg_cap=0, model_image=b"")
    core = WorkerCore.adopt(spec, pipe, src)
    assert pipe.eng.copy_lanes == (2 if ahead else 1)  # the worker asked for the second lane
    prevs, ks = [], []
    for img in imgs:
        assert rb.append_framed(img.framed)
        assert user.push(img.user) == len(img.user) and spans.push(img.spans) == len(img.spans)
        cut = Cut(kernel=rb.producer_pos, user=user.head, spans=spans.head, bases=img.bases)
        rep = core.window(cut, img.n_groups, labels=img.labels)
        ks.append(rep["k"])
        assert src.staged is None and len(core.pending) <= pipe.nb
        prevs.extend(rep["prevs"])
    fin = core.stop()
    prevs.extend(fin["prevs"])
    assert not core.pending and not src.pending and src.staged is None
    assert ks == list(range(len(imgs)))
    done = src.done()
    assert (int(user.tail), int(spans.tail)) == done[1:]
    late = (src.late_dropped, src.resubmitted, src.carried)
    pipe.close()
    return prevs, done, late


def test_worker_returns_the_same_windows_with_and_without_copy_ahead(monkeypatch, replay):
    on, done_on, late_on = _worker_run(monkeypatch, replay, True, "on")
    off, done_off, late_off = _worker_run(monkeypatch, replay, False, "off")
    assert [p["k"] for p in on] == [p["k"] for p in off] == list(range(13))
    for a, b in zip(on, off):
        assert a["packet"].tobytes() == b["packet"].tobytes(), a["k"]
        assert a["ring"].tobytes() == b["ring"].tobytes(), a["k"]
        ra, rb_ = a["results"][0], b["results"][0]
        assert sorted(ra) == sorted(rb_)
        for key in ra:
            assert np.asarray(ra[key]).tobytes() == np.asarray(rb_[key]).tobytes(), (a["k"], key)
        assert math.isfinite(a["latency_ms"]) and a["latency_ms"] >= 0
    assert done_on == done_off and late_on == late_off
    assert any(p["packet"].any() for p in on)


def test_who_keeps_the_plain_order(monkeypatch):
    """A side tracker, the CPU engine and an engine with a communicator stage a window in one piece."""
    from llm_slo_ebpf_toolkit_amd.ops import load_agent
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    monkeypatch.setenv("MISLO_COPY_AHEAD", "1")
    monkeypatch.delenv("MISLO_COPY_LANES", raising=False)
    kw = dict(model="bayes", learn=False, user_cap=USER_CAP)
    plain = WindowPipeline(SIG_CAP, SPAN_CAP, GROUPS, **kw)
    assert plain.eng.copy_ahead and plain.copy_ahead
    plain.close()
    tracked = WindowPipeline(SIG_CAP, SPAN_CAP, GROUPS, sli_sketch=2, **kw)
    assert tracked.eng.copy_ahead and not tracked.copy_ahead
    tracked.close()
    cpu = WindowPipeline(SIG_CAP, SPAN_CAP, GROUPS, engine="cpu", **kw)
    assert not cpu.eng.copy_ahead and not cpu.copy_ahead
    comm = WindowPipeline(SIG_CAP, SPAN_CAP, GROUPS, comm=(load_agent().unique_id(), 0, 1), **kw)
    assert not comm.eng.copy_ahead and not comm.copy_ahead and comm.eng.copy_lanes == 1
    comm.close()
    monkeypatch.setenv("MISLO_WINDOW_OVERLAP", "0")  # the serial chain: nothing to copy ahead of
    serial = WindowPipeline(SIG_CAP, SPAN_CAP, GROUPS, **kw)
    assert not serial.eng.copy_ahead and not serial.copy_ahead
    serial.close()
