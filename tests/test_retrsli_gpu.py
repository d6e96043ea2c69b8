"""The TTFT phase split tracker on the device (ops/csrc/retrsli.hip) against the host implementation
(pipeline/retrsli.py): the same windows through both, step by step -- the whole result block (as bytes), every
field over group_cap and over n_groups, and the resident rolling state must be equal. The named cases of
tests/retrsli_scenarios.py (every bucket edge of both histograms, both sides of every compare, each cell, the
order of the checks, ranks on a lane's last and the next lane's first bucket, n = 1, every verdict and threshold,
age, a service going silent, horizons of two and three windows with a window leaving, empty steps and changing
group counts; one hot key, three adjacent buckets, more keys than the LDS table holds and a randomised run with
the LDS table on and off), the bound helpers, records split over ranges, every refusal, and the whole way through
WindowPipeline and the rings against the host engine."""

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.pipeline import retrsli as rs
from tests import retrsli_scenarios as sc

pytestmark = pytest.mark.gpu


def _pair(cfg, lds=True, **kw):
    from llm_slo_ebpf_toolkit_amd.ops.retrsli import RetrievalSliTracker

    kw = dict(cfg, **kw)
    return RetrievalSliTracker(lds=lds, **kw), rs.RetrievalSliOracle(**kw)


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
        assert (dev.slo_units, dev.budget_units) == (ref.slo_units, ref.budget_units) == (sc.SLO_U, sc.BUDGET_U)
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
def test_hot_keys_with_and_without_the_lds_table(name, lds):
    _run_case(sc.case(name), lds=lds)


def test_the_bound_helpers_are_the_oracle_s():
    from llm_slo_ebpf_toolkit_amd.ops import load_agent

    mod = load_agent()
    assert mod.RETRSLI_LDS_SLOTS == 1024 and mod.RETRSLI_UNIT_MAX == rs.UNIT_MAX and mod.RETRSLI_CELLS == rs.N_CELLS
    rng = np.random.default_rng(2)
    for x in np.concatenate([rng.lognormal(np.log(100.0), 3.0, 300), [0.125, 0.375, 0.625, 0.0, 799.995, 1e7, np.inf]]).astype(np.float32):
        assert mod.retrsli_units_of_ms(float(x)) == int(rs.units_of_ms(x)) == sc.brute_units(x), x
    for b in (200.0, 1e-9, 0.125, 1e12):
        assert mod.retrsli_budget_units(b) == rs.budget_units(b)
    for tb in (False, True):
        for r in (0, sc.BUDGET_U, sc.BUDGET_U + 1, rs.UNIT_MAX):
            for m in (0, sc.SLO_U, sc.SLO_U + 1, rs.UNIT_MAX):
                assert mod.retrsli_cell_of(tb, r, m, sc.SLO_U, sc.BUDGET_U) == sc.brute_cell(tb, r, m, sc.SLO_U, sc.BUDGET_U)
    big = (1 << 32) - 1
    rows = [([big, 0, 0, 0, 0, 0], big, 1, 10 ** 6, 1, 10 ** 6), ([0, 0, 0, 0, big, 0], big, (1 << 31) - 1, 10 ** 6, 999_999, 10 ** 6)]
    for _ in range(200):
        rows.append((rng.integers(0, 30, 6).tolist(), int(rng.integers(0, 200)), int(rng.integers(1, 60)),
                     int(rng.integers(0, 10 ** 6 + 1)), int(rng.integers(1, 10 ** 6)), int(rng.integers(500_001, 10 ** 6 + 1))))
    for c, *args in rows:
        assert mod.retrsli_state_of(c, *args) == rs.state_of(c, *args) == sc.brute_state(c, *args)
    assert (mod.retrsli_age_of(2, 2, 7), mod.retrsli_age_of(2, 3, 7), mod.retrsli_age_of(1, 1, big)) == (8, 1, big)
    for g in (1, 3, 4, 64):
        off = rs.layout(g)
        assert list(mod.retrsli_layout(g)) == [off[k] for k in (*rs.RESULT_FIELDS, "words")]


def test_records_split_over_three_ranges_and_every_refused_step():
    rng = np.random.default_rng(33)
    G = 3
    recs = np.ascontiguousarray(sc.mixed_window(rng, 120, G))
    n = len(recs)
    assert 150 < n <= 256
    a = recs.ctypes.data
    dev, ref = _pair(sc._cfg(span_cap=256))
    try:
        r = _equal_step(dev, ref, recs, G, "three ranges",
                        ranges=[(a, 40 * 64), (a + 40 * 64, 0), (a + 40 * 64, 50 * 64), (a + 90 * 64, (n - 90) * 64)])
        assert int(r["stats"][0]) > 60
        before = dev.resident()
        for bad in (lambda: dev.step([(a, 63)], G), lambda: dev.step_records(recs[:1], 5),
                    lambda: dev.step_records(recs[:1], -1), lambda: dev.step([(a, 200 * 64), (a, 57 * 64)], G),
                    lambda: dev.step([(0, 64)], G)):
            with pytest.raises(ValueError):
                bad()
        for bad in (lambda: ref.step([(a, 63)], G), lambda: ref.step_records(recs[:1], 5),
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
    from llm_slo_ebpf_toolkit_amd.ops.retrsli import RetrievalSliTracker
    from tests.test_retrsli import BAD_CONFIGS

    for kw, _msg in BAD_CONFIGS:
        with pytest.raises(ValueError):
            RetrievalSliTracker(**kw)
        with pytest.raises(ValueError):
            rs.RetrievalSliOracle(**kw)


def test_through_the_pipeline_and_the_rings_equals_the_host_engine():
    rng = np.random.default_rng(41)
    groups = [3, 3, 2, 3, 1, 3]
    wins = [sc.mixed_window(rng, 40, 3) if w != 3 else np.zeros(0, sc.R.SPAN) for w in range(6)]
    gpu, gd = sc.run_pipeline("gpu", wins, groups, 2)
    cpu, cd = sc.run_pipeline("cpu", wins, groups, 2)
    off, _ = sc.run_pipeline("gpu", wins, groups, 0)
    for w, (a, b, c, x, y) in enumerate(zip(gpu, cpu, off, gd, cd)):
        assert set(a) == set(b) == set(c) | set(rs.RESULT_KEYS) and not set(c) & set(rs.RESULT_KEYS)
        sc.same_results(x, y, f"window {w}")
        for key in rs.RESULT_KEYS:
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"window {w} {key}")
        for key in c:  # every other key: the same run with the feature off
            np.testing.assert_array_equal(a[key], c[key], err_msg=f"window {w} {key}")
    assert int(gd[3]["cells"].sum()) == 0 and int(gd[3]["cells_roll"].sum()) > 30
    assert sum(int(r["retr_cells"].sum()) for r in gpu) > 150
