"""The TTFT drift tracker on the device (ops/csrc/drift.hip) against the host implementation
(pipeline/drift.py): the same windows through both, step by step -- the whole result block (as bytes),
every field over group_cap and over n_groups, and the resident state (recent, base, base_fill, base_pos,
hold, ring position) must be equal. The named cases of tests/drift_scenarios.py (identical and disjoint
rows, the maximum on a lane's last and the next lane's first bucket, ties, buckets 0 and 385, both sides
of crit_q, of the shift condition and of every min_* threshold, windows leaving the three rings, empty
windows, withheld and resumed admission, fast, the rebase with stale ring rows, changing group counts, a
silent service; the hot shapes with the LDS table on and off), records split over ranges, every refusal,
and the whole way through WindowPipeline and the rings against the host engine."""

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.pipeline import drift as dr
from tests import drift_scenarios as sc

pytestmark = pytest.mark.gpu


def _pair(cfg, lds=True, **kw):
    from llm_slo_ebpf_toolkit_amd.ops.drift import DriftTracker

    kw = dict(cfg, **kw)
    return DriftTracker(lds=lds, **kw), dr.DriftOracle(**kw)


def _equal_step(dev, ref, recs, G, what, ranges=None):
    i = dev.step_records(recs, G) if ranges is None else dev.step(ranges, G)
    assert i == ref.step_records(recs, G)
    assert dev.block(i).tobytes() == ref.block(i).tobytes(), f"{what}: result blocks differ"
    a, b = dev.results(i, dev.group_cap), ref.results(i, ref.group_cap)
    sc.same_results(a, b, what)
    sc.same_results(dev.results(i, G), ref.results(i, G), what)
    sc.same_resident(dev.resident(), ref.resident(), what)
    return a


def _run_case(c, lds=True):
    dev, ref = _pair(c.cfg, lds=lds)
    seen = []
    try:
        assert dev.crit_q == ref.crit_q and dev.cfg == ref.cfg
        for w, (recs, G) in enumerate(c.steps):
            seen.append(_equal_step(dev, ref, recs, G, f"{c.name} lds={lds} step {w}"))
    finally:
        dev.close()
    if c.check is not None:
        c.check(seen)


@pytest.mark.parametrize("name", [n for n in sc.CASE_NAMES if not n.startswith("hot")])
def test_every_named_case_equals_the_oracle_after_every_step(name):
    _run_case(sc.case(name))


@pytest.mark.parametrize("lds", [True, False])
@pytest.mark.parametrize("name", [n for n in sc.CASE_NAMES if n.startswith("hot")])
def test_hot_shapes_with_and_without_the_lds_table(name, lds):
    _run_case(sc.case(name), lds=lds)


def test_the_device_constants_and_decision_are_the_oracle_s():
    from llm_slo_ebpf_toolkit_amd.ops import load_agent

    mod = load_agent()
    assert mod.DRIFT_LDS_SLOTS == 256 and (mod.DRIFT_K, mod.DRIFT_ROW_STRIDE, mod.DRIFT_PER_LANE) == (386, 392, 7)
    assert (mod.DRIFT_SLOW, mod.DRIFT_FAST, mod.DRIFT_WARMING, mod.DRIFT_REBASED) == (dr.SLOW, dr.FAST, dr.WARMING, dr.REBASED)
    for c2 in (4.0, 5.0, 5.0 - 2.0 ** -32, 1e-12, 0.3, 1e6, 2.0 ** 31, 1e30):
        assert mod.drift_crit_q(c2) == dr.crit_q(c2), c2
    rng = np.random.default_rng(5)
    for _ in range(300):
        n_r, n_b = int(rng.integers(1, 1 << 21)), int(rng.integers(1, 1 << 21))
        sn, fn = int(rng.integers(0, n_r * n_b + 1)), int(rng.integers(0, n_r * n_b + 1))
        qr, qb = sorted(rng.integers(0, 386, 4).tolist()), sorted(rng.integers(0, 386, 4).tolist())
        kw = dict(min_shift=int(rng.integers(0, 4)), min_recent=int(rng.integers(1, 1 << 20)),
                  min_base=int(rng.integers(1, 1 << 20)), min_base_windows=int(rng.integers(1, 5)))
        fill, c2 = int(rng.integers(0, 6)), float(rng.choice([0.5, 4.0, 100.0]))
        assert mod.drift_decide(n_r, n_b, fill, sn, fn, qr, qb, crit=c2, **kw) == \
            dr.decide(n_r, n_b, fill, sn, fn, qr, qb, dr.crit_q(c2), **kw)


def test_records_split_over_three_ranges_and_every_refused_step():
    rng = np.random.default_rng(33)
    G = 3
    recs = np.ascontiguousarray(sc.mixed_window(rng, 120, G, [300.0, 500.0, 80.0]))
    n = len(recs)
    assert 130 < n <= 256
    a = recs.ctypes.data
    dev, ref = _pair(sc._cfg(span_cap=256))
    try:
        r = _equal_step(dev, ref, recs, G, "three ranges",
                        ranges=[(a, 40 * 64), (a + 40 * 64, 0), (a + 40 * 64, 50 * 64), (a + 90 * 64, (n - 90) * 64)])
        assert int(r["stats"][0]) > 90
        before = dev.resident()
        for bad in (lambda: dev.step([(a, 63)], G), lambda: dev.step_records(recs[:1], G + 1),
                    lambda: dev.step_records(recs[:1], -1), lambda: dev.step([(a, 200 * 64), (a, 57 * 64)], G),
                    lambda: dev.step([(0, 64)], G)):
            with pytest.raises(ValueError):
                bad()
        for bad in (lambda: ref.step([(a, 63)], G), lambda: ref.step_records(recs[:1], G + 1),
                    lambda: ref.step_records(recs[:1], -1), lambda: ref.step_records(np.concatenate([recs, recs]), G),
                    lambda: ref.step([(0, 64)], G)):
            with pytest.raises(ValueError):
                bad()
        sc.same_resident(dev.resident(), before, "a refused step changes nothing")
        _equal_step(dev, ref, recs[:17], G, "the step after the refused ones")
        _equal_step(dev, ref, recs[:0], G, "an empty step: no observe launch")
        assert min(dev.step_ms(2)) >= 0.0 and dev.observe_ms(1) >= 0.0 and dev.query(2)
        with pytest.raises(IndexError):
            ref.results(-1, G)
        with pytest.raises(IndexError):
            dev.results(-1, G)
    finally:
        dev.close()


def test_argument_checks():
    from llm_slo_ebpf_toolkit_amd.ops.drift import DriftTracker

    for kw in sc.BAD_CONFIGS:
        with pytest.raises(ValueError):
            DriftTracker(**kw)
        with pytest.raises(ValueError):
            dr.DriftOracle(**kw)


def test_through_the_pipeline_and_the_rings_equals_the_host_engine():
    rng = np.random.default_rng(41)
    groups = [3, 3, 2, 3, 1, 3, 3, 3]
    med = [300.0, 500.0, 80.0]
    wins = [sc.mixed_window(rng, 90, 3, med if w < 5 else [300.0, 900.0, 80.0]) if w != 3 else np.zeros(0, sc.R.SPAN)
            for w in range(8)]
    kw = dict(drift_min_recent=10, drift_min_base=10, drift_min_base_windows=1, drift_hold_max=2)
    gpu, gd = sc.run_pipeline("gpu", wins, groups, (2, 1, 3), **kw)
    cpu, cd = sc.run_pipeline("cpu", wins, groups, (2, 1, 3), **kw)
    off, _ = sc.run_pipeline("gpu", wins, groups, None)
    for w, (a, b, c, x, y) in enumerate(zip(gpu, cpu, off, gd, cd)):
        assert set(a) == set(b) == set(c) | set(dr.RESULT_KEYS) and not set(c) & set(dr.RESULT_KEYS)
        sc.same_results(x, y, f"window {w}")
        for key in dr.RESULT_KEYS:
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"window {w} {key}")
        for key in c:  # every other key: the same run with the feature off
            np.testing.assert_array_equal(a[key], c[key], err_msg=f"window {w} {key}")
    assert int(gd[3]["n_win"].sum()) == 0 and int(gd[3]["n_recent"].sum()) > 30
    states = np.array([r["drift_state"][1] for r in gpu if len(r["drift_state"]) > 1])
    assert (states & dr.SLOW).any() and (states & dr.REBASED).any()
