"""The error SLI tracker on the device (ops/csrc/errsli.hip) against the host implementation
(pipeline/errsli.py): the same windows through both, step by step -- the whole result block (as bytes), every
field over group_cap and over n_groups, and the resident rolling state must be equal. The named cases of
tests/errsli_scenarios.py (every class and the reserved ones, the order of the checks, bad_mask variants,
horizons of two and three windows with a window leaving, one and four pairs, a pair whose windows burn apart,
the compare at equality, min_requests, n = 0, the age, fewer steps than L, L == W, empty steps, changing group
counts and a service going silent; one hot key, more keys than the LDS table places, the second workgroup's
flush and a randomised run with the LDS table on and off), records split over ranges, every refusal, and the
whole way through WindowPipeline and the rings against the host engine."""

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.pipeline import errsli as es
from tests import errsli_scenarios as sc

pytestmark = pytest.mark.gpu


def _pair(cfg, lds=True, **kw):
    from llm_slo_ebpf_toolkit_amd.ops.errsli import ErrorSliTracker

    kw = dict(cfg, **kw)
    return ErrorSliTracker(lds=lds, **kw), es.ErrorSliOracle(**kw)


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
        assert dev.budget_ppm == ref.budget_ppm == sc.BUDGET
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


def test_the_module_s_helpers_are_the_oracle_s():
    from llm_slo_ebpf_toolkit_amd.collector import records as R
    from llm_slo_ebpf_toolkit_amd.ops import load_agent

    mod = load_agent()
    assert mod.ERRSLI_LDS_SLOTS == 256 and mod.ERRSLI_BAD_DEFAULT == es.BAD_DEFAULT
    for c in range(16):
        assert mod.errsli_pack_outcome(c) == R.pack_outcome(c) and mod.errsli_outcome_of(0xFFFFFF0F | (c << 4)) == c
    for t in (0.999, 0.9, 0.99, 0.0, 0.9999999, 0.5):
        assert mod.errsli_budget_ppm(t) == es.budget_ppm(t), t
    top = (1 << 32) - 1
    for n, bad, mn, thr in ((10, 1, 0, 10 ** 8), (11, 1, 0, 10 ** 8), (9, 1, 10, 10 ** 8), (0, 0, 0, 1), (top, top, top, 10 ** 9),
                            (top, top - 1, 0, 10 ** 9), (top, 1, 0, 1)):
        assert mod.errsli_burns(n, bad, mn, thr) == es.burns(n, bad, mn, thr), (n, bad, mn, thr)
    assert mod.errsli_next_age(top, 1) == top and mod.errsli_next_age(5, 0) == 0 and mod.errsli_next_age(5, 2) == 6
    for g in (1, 3, 64, 65536):
        assert dict(mod.errsli_layout(g)) == es.layout(g)
    assert mod.errsli_device_bytes(16384, 64, 3600) == es.device_bytes(16384, 64, 3600)


def test_records_split_over_three_ranges_and_every_refused_step():
    rng = np.random.default_rng(35)
    G = 3
    recs = np.ascontiguousarray(sc.mixed_window(rng, 180, G))
    n = len(recs)
    assert 150 < n <= 256
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
    from llm_slo_ebpf_toolkit_amd.ops.errsli import ErrorSliTracker

    for kw in sc.BAD_CONFIGS:
        with pytest.raises(ValueError):
            ErrorSliTracker(**kw)
        with pytest.raises(ValueError):
            es.ErrorSliOracle(**kw)


def test_through_the_pipeline_and_the_rings_equals_the_host_engine():
    rng = np.random.default_rng(43)
    groups = [3, 3, 2, 3, 1, 3]
    wins = [sc.mixed_window(rng, 40, 3, p_bad=0.3) if w != 3 else np.zeros(0, sc.R.SPAN) for w in range(6)]
    gpu, gd = sc.run_pipeline("gpu", wins, groups, 2)
    cpu, cd = sc.run_pipeline("cpu", wins, groups, 2)
    off, _ = sc.run_pipeline("gpu", wins, groups, 0)
    for w, (a, b, c, x, y) in enumerate(zip(gpu, cpu, off, gd, cd)):
        assert set(a) == set(b) == set(c) | set(es.RESULT_KEYS) and not set(c) & set(es.RESULT_KEYS)
        sc.same_results(x, y, f"window {w}")
        for key in es.RESULT_KEYS:
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"window {w} {key}")
        for key in c:  # every other key: the same run with the feature off
            np.testing.assert_array_equal(a[key], c[key], err_msg=f"window {w} {key}")
    # the empty window's horizon holds window 2 alone (n_groups = 2 there): its finished requests of groups 0 and 1
    w2 = wins[2]
    kept = ((w2["flags"] & 12) == 0) & (w2["group_id"] < 2) & (sc.R.span_outcome(w2["flags"]) < 8)
    assert int(gd[3]["counts"].sum()) == 0 and int(gd[3]["counts_roll"].sum()) == int(kept.sum()) > 15
    assert sum(int(r["err_counts"].sum()) for r in gpu) > 150 and any(int(r["err_firing"].sum()) for r in gpu)
