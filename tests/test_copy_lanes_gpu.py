"""Copy lanes (ops/csrc/engine.hip, ops/csrc/copylanes.h): with two lanes (MISLO_COPY_LANES=2, the
default from four buffers on) window k's DMAs go to copy stream k & 1, so one lane's DMAs are
queued while the other hands a finished window over.

Checked here on the shapes and the stress sequence of tests/test_window_overlap_gpu.py (full, nearly
empty, span-less and event-less windows alternating, staged ahead of the read-back): two lanes
against one lane, byte for byte, for 2 and 3 buffers with graphs on and off; ring ranges that wrap
(two DMA segments) against rings that never wrap; a source left unregistered (pinned staging)
against the registered run; and the order in which copies are reported: ``h2d_done(k)`` means
every window up to k, so "k + 1 done, k not done" is never observed and the rings end up released
by exactly the windows' counts. tests/test_copy_lanes.py holds the lane arithmetic on the host."""

import os
import time

import numpy as np
import pytest

from tests.test_window_overlap_gpu import HALO_MS, SEQUENCE, _feed, _pod_meta, _stress_windows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stress():
    """The stress sequence's ring images and pod table, built once and never changed."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import build_replay_images

    wins, gen = _stress_windows()
    return build_replay_images(wins), _pod_meta(gen)


class _EngNoRegister:
    """The engine, except that it refuses to page-lock the ranges starting at ``addresses``."""

    def __init__(self, eng, addresses):
        self._eng, self._skip = eng, set(addresses)

    def register_host(self, address, nbytes):
        return False if address in self._skip else self._eng.register_host(address, nbytes)

    def __getattr__(self, name):
        return getattr(self._eng, name)


class _PipeNoRegister:
    def __init__(self, pipe, addresses):
        self._pipe, self.eng = pipe, _EngNoRegister(pipe.eng, addresses)

    def __getattr__(self, name):
        return getattr(self._pipe, name)


def _pipeline(lanes, use_graphs=True, n_buffers=3):
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    old = os.environ.get("MISLO_COPY_LANES")
    os.environ["MISLO_COPY_LANES"] = str(lanes)
    try:
        pipe = WindowPipeline(16384, 512, 8, model="bayes", learn=False, user_cap=4096, halo_ms=HALO_MS,
                              use_graphs=use_graphs, n_buffers=n_buffers, max_ahead=n_buffers)
    finally:
        if old is None:
            del os.environ["MISLO_COPY_LANES"]
        else:
            os.environ["MISLO_COPY_LANES"] = old
    assert pipe.eng.copy_lanes == lanes
    return pipe


def _rings(tag, user_slots=1 << 14, span_slots=1 << 12):
    from llm_slo_ebpf_toolkit_amd.runtime import load

    rt = load()
    return (rt.Ringbuf.create_shm(f"/mislo-cl-{os.getpid()}-{tag}", 1 << 22), rt.HostRing(user_slots, 64),
            rt.HostRing(span_slots, 64))


def _run(tag, imgs, pods, lanes, use_graphs=True, n_buffers=3, user_slots=1 << 14, span_slots=1 << 12,
         unregistered=False):
    """The sequence through one engine, windows staged ahead of the read-back: per window the raw
    packet and result block (copies), and what the run saw: ranges that wrapped, staged bytes."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import RingWindowSource

    pipe = _pipeline(lanes, use_graphs, n_buffers)
    rb, user, spans = _rings(tag, user_slots, span_slots)
    src = RingWindowSource(_PipeNoRegister(pipe, [spans.address]) if unregistered else pipe, rb, user, spans)
    assert src.direct == {"ring": True, "user": True, "spans": not unregistered}
    pipe.eng.set_pods(*pods)
    out, ks, seen = [], [], {"wrapped": 0, "n_user": 0, "n_spans": 0}

    def collect(k, n_groups):
        pipe.eng.wait(k)
        res = pipe.eng.results(k, n_groups)
        out.append((np.array(pipe.eng.packet(k), copy=True), {key: np.array(res[key], copy=True) for key in res}))

    for j, img in enumerate(imgs):
        u0, s0 = src.upos, src.spos
        st = src.stage(_feed(img, rb, user, spans), img.n_groups, img.labels)
        ks.append(st["k"])
        seen["n_user"] += st["n_user"]
        seen["n_spans"] += st["n_spans"]
        seen["wrapped"] += int((u0 & (user_slots - 1)) + st["n_user"] > user_slots)
        seen["wrapped"] += int((s0 & (span_slots - 1)) + st["n_spans"] > span_slots)
        if j >= 1:  # window j - 1's host blocks are not rewritten before window j - 1 + n_buffers
            collect(ks[j - 1], imgs[j - 1].n_groups)
    collect(ks[-1], imgs[-1].n_groups)
    src.drain()
    seen["staged"] = int(pipe.eng.staged_bytes)
    seen["released"] = (int(user.tail), int(spans.tail))
    pipe.close()
    return out, seen


def _assert_same(a, b, what):
    assert len(a) == len(b) == len(SEQUENCE)
    for j in range(len(a)):
        msg = f"{what}: window {j} ({SEQUENCE[j]})"
        assert a[j][0].tobytes() == b[j][0].tobytes(), msg
        assert sorted(a[j][1]) == sorted(b[j][1])
        for key in a[j][1]:
            assert a[j][1][key].tobytes() == b[j][1][key].tobytes(), (msg, key)


@pytest.fixture(scope="module")
def one_lane(stress):
    """The one-lane run with 3 buffers and graphs, shared by the tests that compare against it."""
    imgs, pods = stress
    return _run("ref", imgs, pods, 1)


@pytest.mark.parametrize("n_buffers", [2, 3])
@pytest.mark.parametrize("use_graphs", [True, False])
def test_two_lanes_compute_what_one_lane_computes(stress, one_lane, use_graphs, n_buffers):
    imgs, pods = stress
    tag = f"{int(use_graphs)}{n_buffers}"
    one = one_lane if (use_graphs and n_buffers == 3) else _run("a" + tag, imgs, pods, 1, use_graphs, n_buffers)
    two = _run("b" + tag, imgs, pods, 2, use_graphs, n_buffers)
    _assert_same(two[0], one[0], f"graphs {use_graphs}, {n_buffers} buffers")
    assert two[1]["staged"] == 0 and one[1]["staged"] == 0  # every byte straight from the rings
    assert two[1]["released"] == one[1]["released"] == (two[1]["n_user"], two[1]["n_spans"])
    assert any(pk.any() for pk, _ in two[0])


def test_ranges_that_wrap_arrive_as_two_segments(stress, one_lane):
    """Small user and span rings: some windows' ranges wrap and arrive as two DMA segments each,
    placed back to back on the device. Rings large enough for the whole sequence never wrap."""
    imgs, pods = stress
    small = _run("ws", imgs, pods, 2, user_slots=1 << 13)
    large = _run("wl", imgs, pods, 2, user_slots=1 << 17, span_slots=1 << 14)
    assert small[1]["wrapped"] >= 2 and large[1]["wrapped"] == 0, (small[1], large[1])
    _assert_same(small[0], large[0], "wrapped against unwrapped")
    _assert_same(small[0], one_lane[0], "wrapped, two lanes against one")


def test_an_unregistered_source_goes_through_pinned_staging(stress, one_lane):
    """The span ring left unregistered: its bytes are copied to the buffer's pinned staging block
    first (rewritten only after the buffer's previous window was copied, on whichever lane)."""
    imgs, pods = stress
    staged = _run("us", imgs, pods, 2, unregistered=True)
    assert staged[1]["staged"] == 64 * staged[1]["n_spans"] > 0
    _assert_same(staged[0], one_lane[0], "staged spans against the registered run")


def test_default_lane_count_follows_the_buffer_count(monkeypatch):
    """Without MISLO_COPY_LANES: one lane with three buffers, two from four on (docs/BENCHMARKS.md);
    never two without overlapped windows."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    def lanes(n_buffers):
        pipe = WindowPipeline(16384, 512, 8, model="bayes", learn=False, user_cap=4096, n_buffers=n_buffers,
                              max_ahead=n_buffers)
        n = pipe.eng.copy_lanes
        pipe.close()
        return n

    monkeypatch.delenv("MISLO_COPY_LANES", raising=False)
    monkeypatch.delenv("MISLO_WINDOW_OVERLAP", raising=False)
    assert lanes(3) == 1 and lanes(4) == 2
    monkeypatch.setenv("MISLO_COPY_LANES", "2")
    monkeypatch.setenv("MISLO_WINDOW_OVERLAP", "0")
    assert lanes(4) == 1


@pytest.mark.parametrize("lanes", [1, 2])
def test_copies_are_reported_in_window_order(stress, lanes):
    """A large window followed by a tiny one, three windows staged ahead: the tiny window's DMAs
    can end first on the other lane, but h2d_done(k + 1) is never true while h2d_done(k) is false,
    and the rings are released by exactly the windows' record counts."""
    from llm_slo_ebpf_toolkit_amd.pipeline.window import RingWindowSource

    imgs, pods = stress
    big = [img for img, kind in zip(imgs, SEQUENCE) if kind == "F"]
    tiny = [img for img, kind in zip(imgs, SEQUENCE) if kind == "E"]
    assert len(big) >= 6 and len(tiny) >= 6
    pipe = _pipeline(lanes)
    rb, user, spans = _rings(f"o{lanes}")
    src = RingWindowSource(pipe, rb, user, spans)
    pipe.eng.set_pods(*pods)
    eng = pipe.eng
    n_user = n_spans = 0
    ks = []
    deadline = time.monotonic() + 20.0
    assert not eng.h2d_done(0)  # nothing submitted: nothing copied
    for r in range(6):
        for img in (big[r], tiny[r], big[(r + 1) % len(big)]):
            st = src.stage(_feed(img, rb, user, spans), img.n_groups, img.labels)
            ks.append(st["k"])
            n_user += st["n_user"]
            n_spans += st["n_spans"]
        pairs = [(k - 1, k) for k in ks[-3:] if k >= 1]
        open_pairs = list(pairs)
        while open_pairs:
            assert time.monotonic() < deadline, "the copies did not finish"
            for k, k1 in list(open_pairs):
                later, earlier = eng.h2d_done(k1), eng.h2d_done(k)
                assert not (later and not earlier), f"window {k1} reported copied before window {k}"
                if later and earlier:
                    open_pairs.remove((k, k1))
        for k, k1 in pairs:  # and it stays reported
            assert eng.h2d_done(k) and eng.h2d_done(k1)
    assert not eng.h2d_done(ks[-1] + 1)
    src.drain()
    assert (int(user.tail), int(spans.tail)) == (n_user, n_spans)
    assert src.done()[1:] == (n_user, n_spans) and n_user > 0 and n_spans > 0
    pipe.close()
