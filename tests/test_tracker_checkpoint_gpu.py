"""Checkpoint and resume of the side trackers' horizons on the device (ops/csrc/steplane.h snapshot /
restore, docs/TRACKER_CHECKPOINT.md): for each of the eleven trackers an image taken after four steps and
restored into a new tracker, whose later steps equal, as bytes, an uninterrupted device tracker's and the
numpy oracle's; the snapshot enqueued right before a step; the checkpoint kernels' grid-stride path; the
refusals, each of which must leave the tracker as new; and ``WindowPipeline`` with three trackers on over a
``save_checkpoint`` / ``load_checkpoint``. Shapes and steps are tests/test_tracker_checkpoint.py's (horizon 3,
two result buffers, 8 spans, two groups -- ``group_cap=2`` gives 8-byte arrays, the tail case of the 16-byte
path). The refusals are host refusals or a digest mismatch; nothing here asks a kernel for anything but the
lane's own arrays."""

import importlib

import numpy as np
import pytest

from tests.test_steplane_gpu import GROUP_CAP, TRACKERS, same_results
from tests.test_tracker_checkpoint import AFTER, BEFORE, oracle_of, reference

pytestmark = pytest.mark.gpu


def device_of(name, **kw):
    ops = importlib.import_module(f"llm_slo_ebpf_toolkit_amd.ops.{name}")
    return getattr(ops, TRACKERS[name][0])(**kw)


def _agent():
    from llm_slo_ebpf_toolkit_amd.ops import load_agent

    return load_agent()


def _same_resident(a, b, what):
    ra, rb = a.resident(), b.resident()
    if isinstance(ra, dict):
        assert set(ra) == set(rb), what
        ra, rb = [ra[k] for k in sorted(ra)], [rb[k] for k in sorted(rb)]
    flat = lambda r: [y for x in r for y in (flat(x) if isinstance(x, (list, tuple)) else [x])]  # noqa: E731
    fa, fb = flat(ra), flat(rb)
    assert len(fa) == len(fb), what
    for x, y in zip(fa, fb):
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), f"{what}: resident state differs"


@pytest.mark.parametrize("name", list(TRACKERS))
def test_device_round_trip_equals_the_uninterrupted_tracker_and_the_oracle(name):
    kw, steps, later, _saved = reference(name)
    mod = _agent()
    whole, new = device_of(name, **kw), device_of(name, **kw)
    try:
        for w in range(BEFORE):
            assert whole.step_records(steps[w][0], *steps[w][1], GROUP_CAP) == w
        # the snapshot is enqueued, the uninterrupted tracker steps on at once, the image is read afterwards
        ticket = whole.snapshot()
        assert whole.step_records(steps[BEFORE][0], *steps[BEFORE][1], GROUP_CAP) == BEFORE
        image = whole.snapshot_image(ticket)
        assert image.dtype == np.uint8 and len(image) == whole.image_bytes() and len(image) % 16 == 0
        kind, _fp, step, segs, _fields, _host, payload, digest = mod.lane_image_header(image)
        hdr = int(mod.LANE_IMAGE_HEADER_BYTES)
        assert step == BEFORE and payload == sum(segs) == len(image) - hdr and all(s % 16 == 0 for s in segs), (kind, segs)
        assert int(mod.lane_digest(image[hdr:])) == int(digest), "the device's digest is not the host's of the same bytes"
        assert whole.snapshot_kernel_ms() >= 0.0
        assert new.restore(image) == BEFORE
        for i in range(BEFORE):
            with pytest.raises(IndexError):
                new.results(i, GROUP_CAP)  # steps before the resumed index are not held
        for w in range(BEFORE, BEFORE + AFTER):
            recs, extra = steps[w]
            if w > BEFORE:
                assert whole.step_records(recs, *extra, GROUP_CAP) == w
            assert new.step_records(recs, *extra, GROUP_CAP) == w
            got = new.results(w, GROUP_CAP)
            same_results(got, whole.results(w, GROUP_CAP), f"{name} step {w}: restored against uninterrupted")
            same_results(got, later[w - BEFORE], f"{name} step {w}: restored against the oracle")
            if hasattr(new, "block"):
                assert new.block(w).tobytes() == whole.block(w).tobytes(), f"{name} step {w}: result blocks differ"
        if hasattr(new, "resident"):
            _same_resident(new, whole, name)
        with pytest.raises(RuntimeError, match="before the first step"):
            new.restore(image)
    finally:
        whole.close()
        new.close()


def test_snapshot_holds_the_state_before_the_step_that_follows_it():
    """``snapshot()`` and at once ``step()``: the image restored elsewhere is the state before that step (it
    equals a tracker that stopped there), and the step's own results are those of a tracker nobody snapshotted."""
    name = "errsli"
    kw, steps, later, _saved = reference(name)
    a, stopped, plain, b = (device_of(name, **kw) for _ in range(4))
    try:
        for w in range(BEFORE):
            for t in (a, stopped, plain):
                t.step_records(steps[w][0], *steps[w][1], GROUP_CAP)
        ticket = a.snapshot()
        recs, extra = steps[BEFORE + 1]  # a window with records, so that the step changes the horizon
        assert len(recs) and a.step_records(recs, *extra, GROUP_CAP) == plain.step_records(recs, *extra, GROUP_CAP) == BEFORE
        same_results(a.results(BEFORE, GROUP_CAP), plain.results(BEFORE, GROUP_CAP), "the step after a snapshot")
        assert a.block(BEFORE).tobytes() == plain.block(BEFORE).tobytes()
        assert b.restore(a.snapshot_image(ticket)) == BEFORE
        _same_resident(b, stopped, "the image against the tracker that stopped before the step")
        with pytest.raises(AssertionError):
            _same_resident(b, a, "and not the state after it")
    finally:
        for t in (a, stopped, plain, b):
            t.close()


@pytest.mark.parametrize("name", ["retrsli", "decodesli"])
def test_one_workgroup_walks_every_chunk(name):
    """More 16-byte chunks than one workgroup has threads (256), all three checkpoint kernels in one block."""
    kw, steps, later, _saved = reference(name)
    a, b = device_of(name, **kw), device_of(name, **kw)
    try:
        assert (a.image_bytes() - int(_agent().LANE_IMAGE_HEADER_BYTES)) // 16 > 2 * 256  # a workgroup is 256 threads
        a.t.set_checkpoint_blocks(1)
        b.t.set_checkpoint_blocks(1)
        for w in range(BEFORE):
            a.step_records(steps[w][0], *steps[w][1], GROUP_CAP)
        image = a.snapshot_image(a.snapshot())
        hdr = int(_agent().LANE_IMAGE_HEADER_BYTES)
        assert int(_agent().lane_digest(image[hdr:])) == int(_agent().lane_image_header(image)[7])
        assert b.restore(image) == BEFORE
        for w in range(BEFORE, BEFORE + AFTER):
            assert b.step_records(steps[w][0], *steps[w][1], GROUP_CAP) == w
            same_results(b.results(w, GROUP_CAP), later[w - BEFORE], f"{name} step {w}")
        with pytest.raises(ValueError):
            a.t.set_checkpoint_blocks(0)
    finally:
        a.close()
        b.close()


def _is_as_new(name, dev, kw, steps, what):
    """``dev`` steps like a tracker that was never touched: its first step equals a fresh oracle's."""
    fresh = oracle_of(name, **kw)
    recs, extra = steps[0]
    assert dev.step_records(recs, *extra, GROUP_CAP) == fresh.step_records(recs, *extra, GROUP_CAP) == 0, what
    same_results(dev.results(0, GROUP_CAP), fresh.results(0, GROUP_CAP), what)
    recs, extra = steps[1]
    assert dev.step_records(recs, *extra, GROUP_CAP) == fresh.step_records(recs, *extra, GROUP_CAP) == 1, what
    same_results(dev.results(1, GROUP_CAP), fresh.results(1, GROUP_CAP), what)


def test_refusals_leave_the_tracker_as_new():
    name = "errsli"
    kw, steps, later, _saved = reference(name)
    hdr = int(_agent().LANE_IMAGE_HEADER_BYTES)
    src = device_of(name, **kw)
    sk_kw, sk_steps, _l, _s = reference("slisketch")
    sketch = device_of("slisketch", **sk_kw)
    try:
        for w in range(BEFORE):
            src.step_records(steps[w][0], *steps[w][1], GROUP_CAP)
            sketch.step_records(sk_steps[w][0], *sk_steps[w][1], GROUP_CAP)
        image = src.snapshot_image(src.snapshot()).copy()
        other_image = sketch.snapshot_image(sketch.snapshot()).copy()
        assert np.any(image[hdr:]), "a payload of zeros would make the cases below empty"

        flipped = image.copy()
        flipped[hdr + int(np.flatnonzero(image[hdr:])[0])] ^= 0x01
        cases = [("one payload byte flipped", kw, flipped, "digest"),
                 ("truncated by 16 bytes", kw, image[:-16], "bytes, header and payload are"),
                 ("shorter than a header", kw, image[:hdr - 1], "shorter than a header"),
                 ("another tracker's image", kw, other_image, "kind ttft sketch, this tracker error sli"),
                 ("the same kind with another windows", dict(kw, windows=2, pairs=((2, 1, kw["pairs"][0][2]),)), image,
                  "windows 3, this tracker 2"),
                 ("another group_cap", dict(kw, group_cap=GROUP_CAP + 1), image, "group_cap 2, this tracker 3")]
        for what, dev_kw, img, message in cases:
            dev = device_of(name, **dev_kw)
            try:
                with pytest.raises(ValueError, match=message):
                    dev.restore(img)
                _is_as_new(name, dev, dev_kw, steps, what)
            finally:
                dev.close()

        # restore after a step
        dev = device_of(name, **kw)
        try:
            fresh = oracle_of(name, **kw)
            for w in range(2):
                assert dev.step_records(steps[w][0], *steps[w][1], GROUP_CAP) == fresh.step_records(steps[w][0], *steps[w][1],
                                                                                                   GROUP_CAP)
                if w == 0:
                    with pytest.raises(RuntimeError, match="before the first step"):
                        dev.restore(image)
            same_results(dev.results(1, GROUP_CAP), fresh.results(1, GROUP_CAP), "restore after a step")
            # a second snapshot while one is pending; the first is still good, and then a third is taken
            t1 = dev.snapshot()
            with pytest.raises(RuntimeError, match="pending"):
                dev.snapshot()
            first = dev.snapshot_image(t1).copy()
            with pytest.raises(IndexError):
                dev.snapshot_image(t1 + 1)
            t2 = dev.snapshot()
            assert t2 == t1 + 1 and dev.snapshot_image(t2).tobytes() == first.tobytes()
            taker = device_of(name, **kw)
            try:
                assert taker.restore(first) == 2
                for w in range(2, BEFORE):
                    i = taker.step_records(steps[w][0], *steps[w][1], GROUP_CAP)
                    assert i == fresh.step_records(steps[w][0], *steps[w][1], GROUP_CAP) == w
                    same_results(taker.results(w, GROUP_CAP), fresh.results(w, GROUP_CAP), "after the first snapshot")
            finally:
                taker.close()
        finally:
            dev.close()
    finally:
        src.close()
        sketch.close()


class _Pipelines:
    """Pipelines with three trackers on over the ring source, fed the same replay windows."""

    def __init__(self):
        from llm_slo_ebpf_toolkit_amd.pipeline import decodesli, errsli, slisketch
        from llm_slo_ebpf_toolkit_amd.pipeline.window import build_replay_images
        from tests.test_native_engine import pod_meta, windows

        wins, gen = windows(n_win=3, seed=47, n=2000, s=100)
        self.imgs = build_replay_images(wins)
        self.pods = pod_meta(gen)
        self.keys = slisketch.RESULT_KEYS + decodesli.RESULT_KEYS + errsli.RESULT_KEYS
        self.made = []

    def make(self, tag):
        from llm_slo_ebpf_toolkit_amd.pipeline.window import RingWindowSource, WindowPipeline
        from tests.test_native_engine import rings

        # a window of half a minute (the engine's longest is 34 s): none is missed between save and load
        pipe = WindowPipeline(16384, 512, 8, model="bayes", learn=False, user_cap=4096, window_ms=30000.0, sli_sketch=3,
                              decode_sli=3, error_sli=3, error_pairs=((3, 1, 1000),), error_min_requests=0)
        r = rings(tag)
        src = RingWindowSource(pipe, *r)
        pipe.eng.set_pods(*self.pods)
        self.made.append((pipe, src))
        return pipe, src, r

    def run(self, pipe, src, r, i):
        from tests.test_native_engine import feed

        img = self.imgs[i % 3]
        k = src.stage(feed(img, *r), img.n_groups, img.labels)["k"]
        return {key: v for key, v in pipe.results(k, img.n_groups).items() if key in self.keys}

    def close(self):
        for pipe, src in self.made:
            src.drain()
            pipe.close()


def _differ(a, b):
    return any(np.ascontiguousarray(a[k]).tobytes() != np.ascontiguousarray(b[k]).tobytes() for k in a)


def test_window_pipeline_resumes_three_trackers_from_a_checkpoint(tmp_path):
    P = _Pipelines()
    try:
        a, src_a, ra = P.make("tck-a")
        for i in range(4):
            P.run(a, src_a, ra, i)
        src_a.drain()
        path = str(tmp_path / "state.safetensors")
        a.save_checkpoint(path)
        b, src_b, rb = P.make("tck-b")
        meta = b.load_checkpoint(path)
        assert meta["tracker_report"] == {"resumed": ["slisketch", "decodesli", "errsli"], "fresh": {}}
        assert set(meta["trackers"]) == {"slisketch", "decodesli", "errsli"}
        # what makes the comparison mean something: a pipeline that starts fresh differs
        c, src_c, rc = P.make("tck-c")
        for i in range(4, 7):
            want, got = P.run(a, src_a, ra, i), P.run(b, src_b, rb, i)
            assert set(got) == set(P.keys)
            same_results(got, want, f"window {i} after the checkpoint")
            if i == 4:
                assert _differ(P.run(c, src_c, rc, i), want)
    finally:
        P.close()


def test_window_pipeline_makes_up_for_a_missed_window_on_the_device(tmp_path):
    """``now`` one window after the save: every device tracker takes one empty step after its lane restore
    (``t.step([], group_cap)``), as an uninterrupted pipeline's trackers do for a window without spans; with
    three windows missed the horizon of 3 holds nothing and the trackers start fresh."""
    from llm_slo_ebpf_toolkit_amd.utils import checkpoint

    P = _Pipelines()
    try:
        a, src_a, ra = P.make("tgap-a")
        for i in range(4):
            P.run(a, src_a, ra, i)
        src_a.drain()
        path = str(tmp_path / "state.safetensors")
        a.save_checkpoint(path)
        arrays, meta = checkpoint.load(path)
        window_ns = 30_000_000_000
        b, src_b, rb = P.make("tgap-b")
        rep = b.restore(arrays, meta, now_ns=int(meta["saved_unix_ns"]) + window_ns + 1)
        assert rep == {"resumed": ["slisketch", "decodesli", "errsli"], "fresh": {}}
        # the uninterrupted pipeline's window without spans: the same empty step of every tracker
        for t in (a.sketch, a.decode, a.errors):
            t.step([], t.group_cap)
        c, src_c, rc = P.make("tgap-c")  # resumed, but the missed window not made up for
        assert c.restore(arrays, meta, now_ns=int(meta["saved_unix_ns"]))["resumed"] == ["slisketch", "decodesli", "errsli"]
        for i in range(4, 7):
            want, got = P.run(a, src_a, ra, i), P.run(b, src_b, rb, i)
            same_results(got, want, f"window {i} after a missed window")
            if i == 4:
                assert _differ(P.run(c, src_c, rc, i), want), "the empty step changes nothing the test can see"
        d, _src_d, _rd = P.make("tgap-d")
        rep = d.restore(arrays, meta, now_ns=int(meta["saved_unix_ns"]) + 3 * window_ns)
        assert rep["resumed"] == [] and all("3 windows missed, the horizon holds 3" in r for r in rep["fresh"].values())
        assert set(rep["fresh"]) == {"slisketch", "decodesli", "errsli"}
    finally:
        P.close()
