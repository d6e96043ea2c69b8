"""The step lane under every side tracker (ops/csrc/steplane.h) at the edge where a result slot is reused:
each of the eleven Python wrappers with two result buffers, a span buffer of 8 records, two groups and
every other size at its validated minimum, driven five steps beside its numpy oracle -- the smallest
window of the tracker's scenarios in steps 0, 1, 2 and 4, nothing in step 3. After step 4 the steps 4 and
3 (the empty one) are held and equal the oracle's; 2, 0 and 5 are not (IndexError); step 4 is complete
once its results were read; every device time is there and not negative.
tests/test_steplane.py holds the lane's host side on its own."""

import importlib

import numpy as np
import pytest

N_BUFFERS, SPAN_CAP, GROUP_CAP, STEPS, EMPTY_STEP = 2, 8, 2, 5, 3
SECOND_NS = 10 ** 9


def _smallest(windows):
    """The non-empty window with the fewest records (plan() cuts it to the span buffer)."""
    return min((w for w in windows if len(w[0])), key=lambda w: len(w[0]))


def _case_windows(sc):
    return _smallest([s for c in sc.cases() for s in c.steps])


def _made_windows(make):
    rng = np.random.default_rng(11)
    return _smallest([(make(rng, n),) for n in range(1, SPAN_CAP + 1)])


def _stream_windows(sc):
    st = sc.stream(n_groups=GROUP_CAP, per_window=1)
    return _smallest(list(zip(st.windows, st.cuts)))


def _one_pair(w):
    """pair_cap at its minimum of 1 holds one (service, pod) pair a list: the records of the window's first."""
    return w[(w["group_id"] == w["group_id"][0]) & (w["pod_id"] == w["pod_id"][0])]


# name: (wrapper class, oracle class, scenarios module, the sizes at their minimum and what the scenarios'
# records assume, the smallest window -> (records[, cut_ns]), "" / "cut" / "cuts": what a step takes besides the
# records and the group count, values of the native step_ms)
TRACKERS = {
    "openreq": ("OpenRequestTable", "OpenRequestOracle", "openreq_scenarios", lambda sc: dict(cap=64, slo_ms=sc.SLO_MS),
                _stream_windows, "cuts", 2),
    "slisketch": ("SliSketch", "SliSketchOracle", "slisketch_scenarios", lambda sc: dict(windows=1),
                  lambda sc: _made_windows(lambda rng, n: sc.window(rng, n, GROUP_CAP, GROUP_CAP)), "", 2),
    "exemplars": ("ExemplarTracker", "ExemplarOracle", "exemplar_scenarios", lambda sc: dict(k=1, windows=1),
                  lambda sc: _made_windows(lambda rng, n: sc.edge_window(rng, n, GROUP_CAP)), "", 3),
    "podrank": ("PodRankTracker", "PodRankOracle", "podrank_scenarios",
                lambda sc: dict(k=1, windows=1, pair_cap=1, slo_ms=sc.SLO),
                lambda sc: _made_windows(lambda rng, n: _one_pair(sc.edge_window(rng, n, GROUP_CAP))), "", 3),
    "onset": ("OnsetTracker", "OnsetOracle", "onset_scenarios", lambda sc: dict(bins=64), _case_windows, "cut", 3),
    "decodesli": ("DecodeSliTracker", "DecodeSliOracle", "decodesli_scenarios", lambda sc: dict(windows=1), _case_windows, "",
                  3),
    "drift": ("DriftTracker", "DriftOracle", "drift_scenarios", lambda sc: dict(recent=1, gap=1, baseline=1), _case_windows,
              "", 3),
    "errsli": ("ErrorSliTracker", "ErrorSliOracle", "errsli_scenarios",
               lambda sc: dict(windows=1, pairs=((1, 1, sc.F1),), target=sc.TARGET, min_requests=0), _case_windows, "", 3),
    "loadsli": ("LoadSliTracker", "LoadSliOracle", "loadsli_scenarios",
                lambda sc: dict(bins=64, settle_bins=0, recent_bins=1, min_base_bins=1), _case_windows, "cut", 3),
    "satcurve": ("SaturationTracker", "SaturationOracle", "satcurve_scenarios",
                 lambda sc: dict(bins=64, settle_bins=0, recent_bins=1, epoch_bins=64), _case_windows, "cut", 3),
    "retrsli": ("RetrievalSliTracker", "RetrievalSliOracle", "retrsli_scenarios", lambda sc: dict(windows=1), _case_windows,
                "", 3),
}


def plan(name):
    """(configuration, [(records, extra step arguments)] of the five steps) of one tracker."""
    _dev, _ref, scen, cfg, window, takes, _n_ms = TRACKERS[name]
    sc = importlib.import_module(f"tests.{scen}")
    small = window(sc)
    recs = np.ascontiguousarray(small[0][:SPAN_CAP])
    assert 1 <= len(recs) <= SPAN_CAP
    # a step a second: the cut of the scenario's window, then one second later each step
    cut0 = int(small[1]) if takes else SECOND_NS
    steps = []
    for w in range(STEPS):
        cut = cut0 + w * SECOND_NS
        extra = {"": (), "cut": (cut,), "cuts": (cut, cut - SECOND_NS if w else 0)}[takes]
        steps.append((recs[:0] if w == EMPTY_STEP else recs, extra))
    kw = dict(cfg(sc), n_buffers=N_BUFFERS, span_cap=SPAN_CAP, group_cap=GROUP_CAP)
    return kw, steps


def same_results(a, b, what):
    assert set(a) == set(b) and a, what
    for key in a:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, key, x.dtype, y.dtype, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), f"{what}: {key} differs\n{x}\n{y}"  # as bytes: NaN and -0.0 included


def drive(dev, ref, steps, what):
    """The five steps through both; then the two steps that are held, equal."""
    for w, (recs, extra) in enumerate(steps):
        assert dev.step_records(recs, *extra, GROUP_CAP) == ref.step_records(recs, *extra, GROUP_CAP) == w
    last = STEPS - 1
    for i in (last, last - 1):
        same_results(dev.results(i, GROUP_CAP), ref.results(i, GROUP_CAP), f"{what} step {i}")
        if hasattr(dev, "block") and hasattr(ref, "block"):
            assert dev.block(i).tobytes() == ref.block(i).tobytes(), f"{what} step {i}: result blocks differ"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TRACKERS))
def test_five_steps_over_two_result_slots_equal_the_oracle(name):
    ops = importlib.import_module(f"llm_slo_ebpf_toolkit_amd.ops.{name}")
    rules = importlib.import_module(f"llm_slo_ebpf_toolkit_amd.pipeline.{name}")
    dev_cls, ref_cls, _scen, _cfg, _window, _takes, n_ms = TRACKERS[name]
    kw, steps = plan(name)
    dev, ref = getattr(ops, dev_cls)(**kw), getattr(rules, ref_cls)(**kw)
    try:
        drive(dev, ref, steps, name)
        last = STEPS - 1
        assert dev.query(last) is True  # its results were read: the step is complete
        for i in (last, last - 1):
            ms = dev.step_ms(i)
            assert isinstance(ms, tuple) and len(ms) == 2 and min(ms) >= 0.0, (i, ms)
            native = dev.t.step_ms(i)  # (copy + kernels, kernels[, the observe kernel])
            assert isinstance(native, tuple) and len(native) == n_ms and min(native) >= 0.0, (i, native)
        for i in (last - 2, 0, last + 1):
            with pytest.raises(IndexError):
                dev.results(i, GROUP_CAP)
            with pytest.raises(IndexError):
                dev.step_ms(i)
            with pytest.raises(IndexError):
                dev.query(i)
    finally:
        dev.close()
