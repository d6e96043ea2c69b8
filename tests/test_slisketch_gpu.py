"""The TTFT sketch on the device (ops/csrc/slisketch.hip) against the host implementation
(pipeline/slisketch.py): the same windows through both, step by step -- every result array, the
rolling histogram and the window's histogram must be equal. Small windows with the rule's edge
values, horizons that wrap, groups that come and go, contention on one bucket and a spread over
many groups, the capacity's two sides, a randomised run, and the whole way through WindowPipeline
and the rings against the host engine."""

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import slisketch as sk
from tests import slisketch_scenarios as sc

pytestmark = pytest.mark.gpu


def _pair(group_cap, windows, span_cap=16384, **kw):
    from llm_slo_ebpf_toolkit_amd.ops.slisketch import SliSketch

    kw = dict(span_cap=span_cap, group_cap=group_cap, windows=windows, **kw)
    return SliSketch(**kw), sk.SliSketchOracle(**kw)


def _equal_step(dev, ref, recs, G, what, ranges=None):
    i = dev.step_records(recs, G) if ranges is None else dev.step(ranges, G)
    assert i == ref.step_records(recs, G)
    a, b = dev.results(i, G), ref.results(i, G)
    assert set(a) == set(b) == set(sk.RESULT_FIELDS)
    for key in sk.RESULT_FIELDS:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, (what, key)
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what} {key}")
    np.testing.assert_array_equal(dev.rolling(), ref.rolling(), err_msg=f"{what} rolling")
    np.testing.assert_array_equal(dev.window_hist(), ref.window_hist(), err_msg=f"{what} window_hist")
    return a


def _run(dev, ref, wins, groups):
    total = np.zeros(sk.N_STATS, np.int64)
    try:
        for w, (recs, G) in enumerate(zip(wins, groups)):
            total += _equal_step(dev, ref, recs, G, f"step {w}")["stats"].astype(np.int64)
    finally:
        dev.close()
    return sk.stats_dict(total)


def test_small_windows_with_the_edge_values_equal_the_oracle_after_every_step():
    rng = np.random.default_rng(17)
    G = 3
    wins = [sc.window(rng, 40, G, G) for _ in range(8)]
    tot = _run(*_pair(G, 3), wins, [G] * 8)
    n_edge = len(sc.EDGE_VALUES)
    assert tot == {"observed": 8 * (40 + n_edge - 2), "invalid": 16, "underflow": 32, "overflow": 24,
                   "out_of_group": 16}


@pytest.mark.parametrize("W", [1, 2])
def test_horizons_that_wrap_with_an_empty_step_and_a_step_without_groups(W):
    rng = np.random.default_rng(20 + W)
    G = 4
    groups = [G, G, G, 0, G, G]
    wins = [sc.window(rng, n, g, G, edges=n > 20, skipped=n > 0) for n, g in zip((30, 25, 0, 35, 10, 45), groups)]
    assert len(wins[2]) == 0 and len(wins[3]) > 0
    tot = _run(*_pair(G, W), wins, groups)
    assert tot["observed"] > 100 and tot["out_of_group"] >= 10


def test_groups_that_come_and_go_are_still_evicted():
    rng = np.random.default_rng(23)
    groups = [8, 3, 8, 0, 5, 1, 8, 2, 2, 2]
    wins = [sc.window(rng, 60, g, 8, edges=False) for g in groups]
    dev, ref = _pair(8, 3)
    _run(dev, ref, wins, groups)
    assert not ref.rolling()[2:].any() and ref.rolling()[:2].any()  # rows 2..7 left with the horizon


def test_contention_on_one_bucket_and_a_spread_over_many_groups():
    rng = np.random.default_rng(29)
    one = sc.spans(np.full(4096, 437.5), np.zeros(4096, np.int64))
    dev, ref = _pair(4, 2, span_cap=4096)
    try:
        r = _equal_step(dev, ref, one, 4, "one bucket")
        b = int(sk.bucket_of(np.float32(437.5)))
        assert int(r["n"][0]) == 4096 and dev.window_hist()[0, b] == 4096 and (r["q_win"][0] == b).all()
        assert int(r["sum_milli"][0]) == 4096 * 437500 and r["le"][0].tolist() == [0, 0, 0, 0, 4096, 0, 0, 0]
        r = _equal_step(dev, ref, one, 4, "one bucket again")
        assert int(r["n_roll"][0]) == 8192
    finally:
        dev.close()
    C = 1500
    wide = sc.spans(rng.lognormal(np.log(300.0), 1.5, 4096), rng.integers(0, C, 4096))
    dev, ref = _pair(C, 2, span_cap=4096)
    try:
        r = _equal_step(dev, ref, wide, C, "1500 groups")
        assert int(r["n"].sum()) == 4096 and (r["n"] > 0).sum() > 1300
        _equal_step(dev, ref, wide[:100], C - 1, "1500 groups, second step")
    finally:
        dev.close()


def test_exactly_span_cap_over_three_ranges_and_one_more_is_refused():
    rng = np.random.default_rng(31)
    cap, G = 96, 3
    recs = sc.spans(rng.lognormal(np.log(300.0), 1.5, cap + 1), rng.integers(0, G, cap + 1))
    dev, ref = _pair(G, 2, span_cap=cap, n_buffers=2)
    try:
        _equal_step(dev, ref, recs[:50], G, "first")
        full = np.ascontiguousarray(recs[:cap])
        a = full.ctypes.data
        ranges = [(a, 10 * 64), (a + 10 * 64, 0), (a + 10 * 64, 60 * 64), (a + 70 * 64, 26 * 64)]
        r = _equal_step(dev, ref, full, G, "span_cap in three ranges", ranges=ranges)
        assert int(r["n"].sum()) == cap
        before = (dev.rolling(), dev.window_hist(), dev.results(1, G))
        with pytest.raises(ValueError):
            dev.step_records(recs, G)
        with pytest.raises(ValueError):
            ref.step_records(recs, G)
        with pytest.raises(ValueError):
            dev.step([(a, 63)], G)
        with pytest.raises(ValueError):
            dev.step_records(recs[:1], G + 1)
        np.testing.assert_array_equal(dev.rolling(), before[0])
        np.testing.assert_array_equal(dev.window_hist(), before[1])
        for key, v in dev.results(1, G).items():
            np.testing.assert_array_equal(v, before[2][key], err_msg=key)
        assert _equal_step(dev, ref, recs[:5], G, "the step after the refused ones")["n_roll"].sum() == cap + 5
        with pytest.raises(IndexError):
            dev.results(0, G)
        assert min(dev.step_ms(2)) >= 0.0 and dev.query(2)
    finally:
        dev.close()


def test_argument_checks():
    from llm_slo_ebpf_toolkit_amd.ops.slisketch import SliSketch

    for kw in (dict(windows=0), dict(windows=4097), dict(group_cap=0), dict(group_cap=65537), dict(n_buffers=0),
               dict(span_cap=0), dict(span_cap=1 << 20, windows=4096, group_cap=1),
               dict(windows=4096, group_cap=512, span_cap=16)):
        with pytest.raises(ValueError):
            SliSketch(**kw)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_randomised(seed):
    rng = np.random.default_rng(seed)
    C = int(rng.integers(2, 17))
    groups = rng.integers(0, C + 1, 30).tolist()
    wins = [sc.window(rng, int(rng.integers(0, 301)), g, C, edges=bool(rng.integers(0, 2)),
                      skipped=bool(rng.integers(0, 2))) for g in groups]
    tot = _run(*_pair(C, 5, span_cap=512), wins, groups)
    assert tot["observed"] > 1000


def test_through_the_pipeline_and_the_rings_equals_the_host_engine():
    rng = np.random.default_rng(41)
    groups = [3, 3, 2, 3, 1, 3, 3, 3]
    wins = [sc.window(rng, int(n), g, 8, edges=False) for n, g in zip((30, 50, 20, 0, 25, 60, 5, 40), groups)]
    gpu, gsk = sc.run_pipeline("gpu", wins, groups, 3)
    cpu, csk = sc.run_pipeline("cpu", wins, groups, 3)
    for w, (a, b, x, y) in enumerate(zip(gpu, cpu, gsk, csk)):
        assert set(a) == set(b) and set(sk.RESULT_KEYS) <= set(a)
        for key in ("sli", "late") + sk.RESULT_KEYS:
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"window {w} {key}")
        for key in sk.RESULT_FIELDS:
            np.testing.assert_array_equal(x[key], y[key], err_msg=f"window {w} {key}")
        np.testing.assert_array_equal(a["ttft_n"], a["sli"][:, 0] + a["late"][:, 0], err_msg=f"window {w}")
    assert sum(int(r["ttft_n"].sum()) for r in gpu) > 150
