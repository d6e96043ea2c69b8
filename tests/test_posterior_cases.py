"""The crafted posterior / statistics / refit cases (tests/posterior_cases.py) deserve the assertions
tests/test_posterior_gpu.py makes about them: every compared top-1 has a clear margin in the
reference itself (no row is left out to get it), exact sums are exactly representable, every
threshold has rows on both sides, and the float32 model image scores every case as the model does."""

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.models.bayes import soft_labels
from llm_slo_ebpf_toolkit_amd.signals import catalog
from tests import posterior_cases as pc


@pytest.mark.parametrize("name", pc.score_cases())
def test_reference_is_decisive_finite_and_normalised(name):
    case, ref = pc.cases()[name], pc.reference(pc.cases()[name])
    assert case.feat.dtype == np.float32 and case.feat.shape == (case.n, 16)
    assert ref.post.shape == (case.n, 10) and np.isfinite(ref.post).all()
    if case.tie:
        assert (ref.gap == 0.0).all()                       # bitwise-equal leaders, every row
        assert (ref.pred == pc.TIE_LOW).all()               # the lowest index of the two
        np.testing.assert_array_equal(ref.post[:, pc.TIE_LOW], ref.post[:, pc.TIE_HIGH])
    else:
        assert ref.gap.min() >= pc.MIN_GAP, (name, float(ref.gap.min()), int(ref.gap.argmin()))
    if case.model.pairs is None:
        np.testing.assert_allclose(ref.post.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    else:  # marginals: a pair counts for both members
        assert (ref.post.sum(axis=1) >= 1.0 - 1e-12).all() and (ref.post.sum(axis=1) <= 2.0 + 1e-12).all()


@pytest.mark.parametrize("name", pc.score_cases())
def test_model_image_round_trip_scores_identically(name):
    """MODEL_DTYPE keeps thresholds in float32: shipped thresholds are small integers, so the image
    scores every case exactly as the model it was made from."""
    case = pc.cases()[name]
    a, b = pc.reference(case), pc.reference_unrounded(case)
    np.testing.assert_array_equal(a.post, b.post)
    np.testing.assert_array_equal(a.pred, b.pred)
    np.testing.assert_array_equal(a.evbits, b.evbits)


def test_row_count_cases_cover_every_group_and_block_edge():
    for kind, tiles in (("ref", 0), ("gpu", 0), ("pairs36", 3), ("pairs16", 1)):
        for n in pc.ROW_COUNTS:
            case = pc.cases()[f"rows-{kind}-{n}"]
            assert case.n == n
            P = 0 if case.model.pairs is None else len(case.model.pairs)
            assert (P + 15) // 16 == tiles
            if n >= 15:
                assert 0.2 < np.isnan(case.feat).mean() < 0.4
    assert max(pc.ROW_COUNTS) > 64 and {15, 16, 17, 63, 64, 65} <= set(pc.ROW_COUNTS)


def test_lda_cases_run_the_continuous_branch():
    for name in ("lda-fixture", "lda-random"):
        case = pc.cases()[name]
        assert case.model.feature_mode == "continuous" and case.model.mean is not None
        assert np.isnan(case.feat).any() and not np.isinf(case.feat).any()  # log1p(inf): a NaN reference
    f = pc.cases()["lda-random"].feat
    assert f.shape[0] == 129 and (f == 0).any() and (f < 0).any() and pc.cases()["lda-fixture"].n == 55


@pytest.mark.parametrize("name", ["thr-gpu", "thr-marginalized"])
def test_threshold_cases_sit_on_both_sides_of_every_threshold(name):
    case = pc.cases()[name]
    f = case.feat
    for s in range(16):
        t = pc.THR32[s]
        assert np.float64(t) == catalog.SIGNALS[s].elevated      # float32 holds the shipped threshold
        col = f[8 * s:8 * s + 8, s]
        assert col[0] == t and col[1] < t and col[2] > t
        assert np.nextafter(col[1], np.float32(np.inf)) == t and np.nextafter(t, np.float32(np.inf)) == col[2]
        assert np.isposinf(col[3]) and np.isneginf(col[4]) and col[5] == 0 and np.signbit(col[5]) and col[6] < 0
        assert 0 < col[7] < np.finfo(np.float32).tiny
        raw = col >= t
        assert raw.tolist() == [True, False, True, True, False, False, False, False]
    assert np.isnan(f[-1]).all()
    ref = pc.reference(case)
    if name == "thr-marginalized":
        dropped = [s for s in range(16) if not case.model.table_mask[s]]
        assert dropped == list(pc.DROPPED_SLOTS)
        for s in dropped:                                       # a dropped slot is never evidence
            assert not ((ref.evbits >> np.uint32(s)) & 1).any()
    else:  # the elevated neighbours show as evidence of some domain, the others of none
        for s in range(16):
            bit = ((ref.evbits[8 * s:8 * s + 8] >> np.uint32(s)) & 1).any(axis=1)
            assert bit.tolist() == [True, False, True, True, False, False, False, False]
    assert not ref.evbits[-1].any()


def test_special_models():
    one = pc.cases()["single-active"]
    ref = pc.reference(one)
    assert np.isfinite(one.model.bias).sum() == 1 and (ref.pred == 5).all() and (ref.post[:, 5] == 1.0).all()
    under = pc.reference(pc.cases()["underflow"])
    losers = np.sort(under.post, axis=1)[:, :-1]
    assert (losers == 0.0).all() and (under.post.max(axis=1) == 1.0).all()
    tie = pc.cases()["tie"].model
    assert 0 < pc.TIE_LOW < pc.TIE_HIGH
    np.testing.assert_array_equal(tie.weights[:, pc.TIE_LOW], tie.weights[:, pc.TIE_HIGH])
    assert tie.bias[pc.TIE_LOW] == tie.bias[pc.TIE_HIGH]
    assert (tie.weights * 64 == np.round(tie.weights * 64)).all()  # exact sums in any order


def test_label_case_mixes_unlabelled_rows_and_a_primary_beyond_the_matrix():
    case = pc.cases()["labels"]
    y = case.labels
    assert (y == -1).sum() >= 20 and set(range(10)) <= set((y[y >= 0] & 0xFF).tolist())
    assert ((y >= 0) & ((y & 0xFF) >= 16)).sum() == 1
    ref = pc.reference(case)
    assert ref.confusion.sum() == (y >= 0).sum() - 1


@pytest.mark.parametrize("name", ["app-single", "app-pairs"])
def test_application_cases_hit_the_threshold_and_share_row_groups(name):
    case = pc.cases()[name]
    ref = pc.reference(case)
    resid = case.model.app.residual(case.app_cnt, case.feat)
    assert (resid[ref.state == 1] >= pc.APP_THR_MS).all()
    assert (resid == pc.APP_THR_MS).sum() >= 4                       # exactly at the threshold: elevated
    just = resid[(ref.state == 0)]
    assert len(just) >= 4 and (just < pc.APP_THR_MS).all() and (just > pc.APP_THR_MS - 0.011).all()
    for g in (ref.state[:16], ref.state[16:]):                       # absent beside present in a row group
        assert (g == -1).any() and (g >= 0).any()
    for s in (0, 3, 5):
        assert np.isnan(case.feat[ref.state >= 0, s]).any()
    assert (name == "app-pairs") == (case.model.pairs is not None)
    assert ((ref.evbits >> np.uint32(16)) & 1).any()


@pytest.mark.parametrize("name", pc.stats_cases())
def test_statistics_cases_have_exactly_summable_label_masses(name):
    case = pc.cases()[name]
    assert set(np.unique(case.weights).tolist()) <= {0.25, 0.5, 1.0, 2.0}
    on = case.labels >= 0
    assert (~on).any() and on.any()
    sizes = {bin((int(c) >> 8) & 0xFFFF).count("1") or 1 for c in case.labels[on]}
    assert sizes <= {1, 2, 4} and (case.n < 50 or sizes == {1, 2, 4})
    Y = soft_labels(case.labels[on], 16) * case.weights.astype(np.float64)[on, None]
    assert (Y * 16 == np.round(Y * 16)).all()                        # multiples of 1/16: dyadic
    for lo in range(0, case.n, 256):                                 # every wave of k_stats contributes
        chunk = on & (np.arange(case.n) >= lo) & (np.arange(case.n) < lo + 256)
        assert soft_labels(case.labels[chunk], 16).any(), lo
    out, count = pc.stats_reference(case)
    # exact in any order: the same sums in extended precision and in reverse order
    np.testing.assert_array_equal(count, Y[::-1].sum(axis=0))
    np.testing.assert_array_equal(count, Y.astype(np.longdouble).sum(axis=0).astype(np.float64))
    assert (out[:16, :16] * 16 == np.round(out[:16, :16] * 16)).all()
    assert out.shape == (32, 32) and np.isfinite(out).all() and (out >= 0).all()
    assert out[:16, 16:].any() and count[10:].sum() == 0
    np.testing.assert_array_equal(out[16:, 16:], out[16:, 16:].T)


def test_refit_cases_deactivate_what_they_should():
    zero, only = pc.refit_cases()["zero-mass"], pc.refit_cases()["only-capped"]
    for pairs in (False, True):
        m = zero.host(pairs)
        assert np.isneginf(m.bias[pc.ZERO_DOM]) and np.isfinite(np.delete(m.bias, pc.ZERO_DOM)).all()
        if pairs:
            hit = (m.pairs[:, 0] == pc.ZERO_DOM) | (m.pairs[:, 1] == pc.ZERO_DOM)
            assert hit.sum() == 8 and np.isneginf(m.pair_b[hit]).all() and not m.pair_w[:, hit].any()
            assert np.isfinite(m.pair_b[~hit]).all()
        o = only.host(pairs)
        assert np.isfinite(o.bias).sum() == 1 and np.isfinite(o.bias[pc.UNKNOWN])
        if pairs:
            assert np.isneginf(o.pair_b).all() and not o.pair_w.any()
    # the cap bites where other domains are active, and cannot where none is
    from llm_slo_ebpf_toolkit_amd.models.bayes import NaiveBayes

    for case, bites in ((zero, True), (only, False)):
        free = NaiveBayes.learned(case.stats, temperature=case.temperature, **dict(case.kwargs, cap_domain=None))
        capped = case.host(False)
        assert (capped.bias[pc.UNKNOWN] < free.bias[pc.UNKNOWN]) == bites
        assert bites or capped.bias[pc.UNKNOWN] == free.bias[pc.UNKNOWN]
    assert zero.packed().shape == (1040,) and zero.p0().shape == (2, 16, 16) and zero.p0()[1].any()
