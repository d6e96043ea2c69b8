"""The request-exemplar tracker on the device (ops/csrc/exemplars.hip) against the host implementation
(pipeline/exemplars.py): the same windows through both, step by step -- every result array and the
resident horizon must be equal, rows compared as bytes. Small windows with the order's edge values,
horizons that wrap, contention on one group in every arrival order, a spread over both sides of the
LDS group limit, indices that run across ranges, the capacity's two sides, a randomised run, and the
whole way through WindowPipeline and the rings against the host engine."""

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.collector import records as R
from llm_slo_ebpf_toolkit_amd.pipeline import exemplars as ex
from tests import exemplar_scenarios as sc

pytestmark = pytest.mark.gpu


def _pair(k, windows, group_cap, span_cap=16384, **kw):
    from llm_slo_ebpf_toolkit_amd.ops.exemplars import ExemplarTracker

    kw = dict(k=k, windows=windows, span_cap=span_cap, group_cap=group_cap, **kw)
    return ExemplarTracker(**kw), ex.ExemplarOracle(**kw)


def _same_resident(dev, ref, what):
    a, b = dev.resident(), ref.resident()
    sc.same_rows(a["rows"], b["rows"], f"{what} resident rows")
    assert a["k"].dtype == b["k"].dtype
    np.testing.assert_array_equal(a["k"], b["k"], err_msg=f"{what} resident counts")


def _equal_step(dev, ref, recs, G, what, ranges=None):
    i = dev.step_records(recs, G) if ranges is None else dev.step(ranges, G)
    assert i == ref.step_records(recs, G)
    # every row of group_cap: a group absent from the step still ages
    a, b = dev.results(i, dev.group_cap), ref.results(i, ref.group_cap)
    sc.same_results(a, b, what)
    sc.same_results(dev.results(i, G), ref.results(i, G), what)
    _same_resident(dev, ref, what)
    return a


def _run(dev, ref, wins, groups):
    total = np.zeros(ex.N_STATS, np.int64)
    try:
        for w, (recs, G) in enumerate(zip(wins, groups)):
            total += _equal_step(dev, ref, recs, G, f"step {w}")["stats"].astype(np.int64)
    finally:
        dev.close()
    return ex.stats_dict(total)


@pytest.mark.parametrize("K", [1, 3, 8])
def test_small_windows_with_the_edge_values_equal_the_oracle_after_every_step(K):
    rng = np.random.default_rng(17 + K)
    G = 3
    wins = [sc.edge_window(rng, 40, G) for _ in range(8)]
    tot = _run(*_pair(K, 3, G), wins, [G] * 8)
    n_edge = len(sc.EDGE_TTFT)
    # per window: 40 + the edge values of 3 groups, 2 of them invalid each; 2 records out of group
    assert tot == {"observed": 8 * (40 + 3 * (n_edge - 2)), "invalid": 8 * 3 * 2, "out_of_group": 16}


@pytest.mark.parametrize("H", [1, 2])
def test_horizons_that_wrap_with_an_empty_step_and_a_step_without_groups(H):
    rng = np.random.default_rng(20 + H)
    G = 4
    groups = [G, G, G, 0, G, G]
    wins = [sc.identify(sc.window(rng, n, g, G, edges=n > 20, skipped=n > 0), rng)
            for n, g in zip((30, 25, 0, 35, 10, 45), groups)]
    assert len(wins[2]) == 0 and len(wins[3]) > 0
    dev, ref = _pair(3, H, G)
    tot = _run(dev, ref, wins, groups)
    assert tot["observed"] > 100 and tot["out_of_group"] >= 10
    # steps 2 (empty) and 3 (no groups) fill a horizon of up to two windows with nothing
    assert not ref.results(3, G)["k_recent"].any() and ref.results(4, G)["k_recent"].any()


def test_contention_on_one_group_the_first_k_indices_win():
    one = sc.identify(sc.spans(np.full(4096, 437.5), np.zeros(4096, np.int64)), np.random.default_rng(1))
    for K in (1, 3, 8):
        dev, ref = _pair(K, 2, 4, span_cap=4096)
        try:
            r = _equal_step(dev, ref, one, 4, f"one group K={K}")
            assert int(r["n"][0]) == 4096 and r["win"][0]["index"].tolist() == list(range(K))
            r = _equal_step(dev, ref, one[::-1], 4, f"one group again K={K}")
            assert r["recent"][0]["age"].tolist() == [0] * K  # equal TTFTs: the newer window's
            sc.same_rows(r["win"][0], ex.rows_of(one[::-1], np.arange(K)))
        finally:
            dev.close()


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_distinct_values_in_every_arrival_order_lose_no_key_to_the_skip_read(order):
    v = 100.0 + np.arange(4096, dtype=np.float32) * np.float32(0.25)  # exact in float32, all distinct
    v = v if order == "ascending" else v[::-1]
    recs = sc.identify(sc.spans(v, np.zeros(4096, np.int64)), np.random.default_rng(2))
    best = np.argsort(-v.astype(np.float64), kind="stable")
    for K, lds in ((8, True), (3, True), (8, False)):
        from llm_slo_ebpf_toolkit_amd.ops.exemplars import ExemplarTracker

        dev = ExemplarTracker(k=K, windows=2, span_cap=4096, group_cap=2, lds=lds)
        ref = ex.ExemplarOracle(k=K, windows=2, span_cap=4096, group_cap=2)
        try:
            r = _equal_step(dev, ref, recs, 1, f"{order} K={K} lds={lds}")
            assert r["win"][0]["index"].tolist() == best[:K].tolist()
            assert r["win"][0]["ttft_ms"][0] == np.float32(100.0 + 4095 * 0.25)
        finally:
            dev.close()


def test_a_spread_over_both_sides_of_the_lds_group_limit():
    rng = np.random.default_rng(29)
    C = 512
    grp = rng.integers(0, C, 2048)
    dev, ref = _pair(3, 2, C, span_cap=2048)
    L = dev.lds_groups
    assert 0 < L < C
    grp[:24] = np.repeat([L - 1, L, L + 1], 8)  # the groups on, at and past the limit hold more than K
    wide = sc.identify(sc.spans(rng.lognormal(np.log(300.0), 1.5, 2048), grp), rng)
    try:
        r = _equal_step(dev, ref, wide, C, "512 groups")
        assert int(r["n"].sum()) == 2048 and (r["n"] > 0).sum() > 480 and (r["k_win"][L - 1:L + 2] == 3).all()
        # n_groups on the limit, one below and one above it: the LDS table's last group, and none beyond
        for G in (L, L - 1, L + 1):
            r = _equal_step(dev, ref, wide[:600], G, f"n_groups = {G}")
            assert int(r["stats"][2]) == int((wide["group_id"][:600] >= G).sum()) > 0
    finally:
        dev.close()


def test_two_and_three_ranges_in_one_step_indices_run_across_ranges():
    rng = np.random.default_rng(33)
    G = 3
    recs = np.ascontiguousarray(sc.identify(sc.window(rng, 90, G, G, edges=False, skipped=False), rng))
    a = recs.ctypes.data
    dev, ref = _pair(3, 2, G, span_cap=128)
    try:
        r = _equal_step(dev, ref, recs, G, "two ranges", ranges=[(a, 40 * 64), (a + 40 * 64, 50 * 64)])
        assert (r["win"]["index"] >= 40).any() and int(r["n"].sum()) == 90
        # out of order and with an empty range: the index is the position in the ranges as given
        order = np.concatenate([np.arange(60, 90), np.arange(0, 25), np.arange(25, 60)])
        ranges = [(a + 60 * 64, 30 * 64), (a, 25 * 64), (a + 25 * 64, 0), (a + 25 * 64, 35 * 64)]
        r = _equal_step(dev, ref, recs[order], G, "three ranges", ranges=ranges)
        assert (r["win"]["index"] >= 55).any()
    finally:
        dev.close()


def test_exactly_span_cap_and_one_more_is_refused_with_the_state_unchanged():
    rng = np.random.default_rng(31)
    cap, G = 96, 3
    recs = sc.identify(sc.spans(rng.lognormal(np.log(300.0), 1.5, cap + 1), rng.integers(0, G, cap + 1)), rng)
    dev, ref = _pair(3, 2, G, span_cap=cap, n_buffers=2)
    try:
        _equal_step(dev, ref, recs[:50], G, "first")
        r = _equal_step(dev, ref, recs[:cap], G, "span_cap exactly")
        assert int(r["n"].sum()) == cap
        before = (dev.resident(), dev.results(1, G))
        with pytest.raises(ValueError):
            dev.step_records(recs, G)
        with pytest.raises(ValueError):
            ref.step_records(recs, G)
        with pytest.raises(ValueError):
            dev.step([(recs.ctypes.data, 63)], G)
        with pytest.raises(ValueError):
            dev.step_records(recs[:1], G + 1)
        after = dev.resident()
        sc.same_rows(after["rows"], before[0]["rows"], "refused steps")
        np.testing.assert_array_equal(after["k"], before[0]["k"])
        sc.same_results(dev.results(1, G), before[1], "refused steps")
        _equal_step(dev, ref, recs[:5], G, "the step after the refused ones")
        with pytest.raises(IndexError):
            dev.results(0, G)
        assert min(dev.step_ms(2)) >= 0.0 and dev.select_ms(2) >= 0.0 and dev.query(2)
    finally:
        dev.close()


def test_argument_checks():
    from llm_slo_ebpf_toolkit_amd.ops.exemplars import ExemplarTracker

    for kw in (dict(k=0), dict(k=9), dict(windows=0), dict(windows=17), dict(group_cap=0), dict(group_cap=65537),
               dict(span_cap=0), dict(span_cap=1 << 31), dict(n_buffers=0), dict(n_buffers=65)):
        with pytest.raises(ValueError):
            ExemplarTracker(**kw)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_randomised_with_n_groups_changing(seed):
    rng = np.random.default_rng(seed)
    C = int(rng.integers(2, 17)) if seed < 3 else 90  # the last one past the LDS group limit
    K, H = int(rng.integers(1, 9)), int(rng.integers(1, 6))
    groups = rng.integers(0, C + 1, 30).tolist()
    wins = [sc.identify(sc.window(rng, int(rng.integers(0, 301)), g, C, edges=bool(rng.integers(0, 2)),
                                  skipped=bool(rng.integers(0, 2))), rng) for g in groups]
    tot = _run(*_pair(K, H, C, span_cap=512), wins, groups)
    assert tot["observed"] > 1000


def test_through_the_pipeline_and_the_rings_equals_the_host_engine():
    rng = np.random.default_rng(41)
    groups = [3, 3, 2, 3, 1, 3]
    wins = [sc.identify(sc.window(rng, int(n), g, 8, edges=False), rng)
            for n, g in zip((30, 50, 20, 0, 25, 60), groups)]
    gpu, gex = sc.run_pipeline("gpu", wins, groups, 3)
    cpu, cex = sc.run_pipeline("cpu", wins, groups, 3)
    off, _ = sc.run_pipeline("gpu", wins, groups, 0)
    for w, (a, b, c, x, y) in enumerate(zip(gpu, cpu, off, gex, cex)):
        assert set(a) == set(b) == set(c) | set(ex.RESULT_KEYS)
        for key in ("ex_n", "ex_k_win", "ex_k_recent"):
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"window {w} {key}")
        for key in ("ex_win", "ex_recent"):
            sc.same_rows(a[key], b[key], f"window {w} {key}")
        sc.same_results(x, y, f"window {w}")
        for key in c:  # every other key: the same run with the feature off
            np.testing.assert_array_equal(a[key], c[key], err_msg=f"window {w} {key}")
        np.testing.assert_array_equal(a["ex_n"], a["sli"][:, 0] + a["late"][:, 0], err_msg=f"window {w}")
    assert sum(int(r["ex_n"].sum()) for r in gpu) > 150
