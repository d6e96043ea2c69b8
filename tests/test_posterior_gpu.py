"""K3 on the device (ops/csrc/posterior.hip: k_posterior, k_stats, k_posterior_stats, k_refit_nb)
against the float64 references of tests/posterior_cases.py on crafted rows: continuous mode (LDA),
more than one block and wave, weights, the E^T X block, the confidence output, G < cap, the fused
launch against the standalone ones, threshold edges, exact argmax ties, label and application
evidence edges, and refits with inactive domains and pairs.

Two entry points: the shipped WindowEngine's ``score(feat, labels, app)`` for any row count, and
the kernel harness' torch ``Engine`` with features written straight into its buffers for everything
else (statistics, the fused launch, a row count below the capacity, refit_nb)."""

import numpy as np
import pytest

from llm_slo_ebpf_toolkit_amd.models.bayes import NaiveBayes, SufficientStats, with_pairs
from llm_slo_ebpf_toolkit_amd.ops.engine import MODEL_DTYPE, app_model_bytes, model_bytes
from llm_slo_ebpf_toolkit_amd.signals import catalog
from tests import posterior_cases as pc

pytestmark = pytest.mark.gpu

EVBITS_SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def pipe():
    from llm_slo_ebpf_toolkit_amd.pipeline.window import WindowPipeline

    p = WindowPipeline(4096, 64, 4, model="bayes_gpu", learn=False, user_cap=64)
    yield p
    p.eng.close()


@pytest.fixture(scope="module")
def small():
    from llm_slo_ebpf_toolkit_amd.ops.engine import KernelHarness

    return KernelHarness(sig_cap=256, span_cap=64, group_cap=64)


@pytest.fixture(scope="module")
def big():
    from llm_slo_ebpf_toolkit_amd.ops.engine import KernelHarness

    return KernelHarness(sig_cap=256, span_cap=64, group_cap=1100)


def _bits(a):
    """float64 array as its bit patterns: equality that tells -0.0 from 0.0 and compares NaNs."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_rows(case, ref, post, pred, conf, evbits, rows=None):
    """The posterior kernel's outputs of the first ``rows`` rows against the reference."""
    n = case.n if rows is None else rows
    post, pred, conf, evbits = post[:n], pred[:n], conf[:n], np.asarray(evbits[:n]).view(np.uint32)
    err = np.abs(post[:, :10] - ref.post[:n])
    print(f"{case.name}: rows {n} max |post - ref| {err.max():.3e} min ref gap {ref.gap[:n].min():.3e}")
    np.testing.assert_allclose(post[:, :10], ref.post[:n], rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(pred, ref.pred[:n])
    np.testing.assert_array_equal(evbits[:, :10], ref.evbits[:n])
    assert not post[:, 10:].any() and not evbits[:, 10:].any()          # the padded domains
    np.testing.assert_array_equal(_bits(conf), _bits(post[np.arange(n), pred]))  # the same register
    if case.model.pairs is None:
        np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    if case.tie:
        assert (pred == pc.TIE_LOW).all()
        np.testing.assert_array_equal(_bits(post[:, pc.TIE_LOW]), _bits(post[:, pc.TIE_HIGH]))


# ---- the shipped engine's score() ---------------------------------------------------------------
@pytest.mark.parametrize("name", pc.score_cases())
def test_score_matches_the_reference(pipe, name):
    """Row counts across every row-group and block edge for 0 / 1 / 3 pair tiles, LDA (continuous
    mode), threshold edges with and without a table mask, an exact tie, a single active domain,
    underflowing losers, label edge cases (confusion) and application-evidence edges."""
    case = pc.cases()[name]
    ref = pc.reference(case)
    pipe.eng.set_model_bytes(model_bytes(case.model))
    if case.app_cnt is not None:
        pipe.eng.set_app_model(app_model_bytes(case.model))
    out = pipe.eng.score(case.feat, case.labels, case.app_cnt)
    check_rows(case, ref, out["post"], out["pred"], out["conf"], out["evbits"])
    if case.labels is not None:
        np.testing.assert_array_equal(out["confusion"].astype(np.int64), ref.confusion)
    if case.app_cnt is not None:
        assert set(ref.state.tolist()) == {-1, 0, 1}


# ---- the kernel harness: injected features ------------------------------------------------------
def load_rows(h, feat, labels, G):
    torch, e = h.torch, h.eng
    n = len(feat)
    assert n <= h.group_cap and G <= h.group_cap
    e.feat.fill_(float("nan"))
    e.feat[:n].copy_(torch.from_numpy(np.ascontiguousarray(feat, dtype=np.float32)).to(h.device))
    e.labels.fill_(-1)
    if labels is not None:
        e.labels[:n].copy_(torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).to(h.device))
    e.counts[2:3].fill_(int(G))


def outputs(h, n):
    e = h.eng
    h.torch.cuda.synchronize(h.device)
    return {"post": e.post[:n].cpu().numpy(), "pred": e.pred[:n].cpu().numpy(), "conf": e.gconf[:n].cpu().numpy(),
            "evbits": e.evbits[:n].cpu().numpy().view(np.uint32), "confusion": e.confusion.cpu().numpy().astype(np.int64),
            "stats": e.stats.cpu().numpy(), "count": e.stats_count.cpu().numpy()}


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", ["gpu", "pairs36"])
@pytest.mark.parametrize("G", [1, 17, 40])
def test_rows_beyond_the_count_are_left_untouched(small, G, kind, fused):
    """G = min(*ng_ptr, cap) < cap: the first G rows are scored, every later row of every output
    keeps what it held."""
    case = pc.cases()[f"rows-{kind}-64"]
    ref = pc.reference(case)
    e = small.eng
    small.set_model(case.model)
    load_rows(small, case.feat, None, G)
    e.post.fill_(-7.0)
    e.pred.fill_(-9)
    e.gconf.fill_(-5.0)
    e.evbits.fill_(EVBITS_SENTINEL)
    e.reset_window()
    if fused:
        e.posterior_and_stats(False)
    else:
        e.posterior(False)
    out = outputs(small, 64)
    check_rows(case, ref, out["post"], out["pred"], out["conf"], out["evbits"], rows=G)
    assert (out["post"][G:] == -7.0).all() and (out["pred"][G:] == -9).all() and (out["conf"][G:] == -5.0).all()
    assert (out["evbits"][G:] == EVBITS_SENTINEL).all()
    assert not out["confusion"].any()                                       # no labels given


def _labels_for(case):
    return case.labels if case.labels is not None else pc.label_codes(500 + case.n, case.n)


@pytest.mark.parametrize("name", ["labels", "rows-pairs36-129", "rows-pairs16-65", "lda-random", "rows-gpu-129", "tie"])
def test_fused_launch_equals_the_standalone_launches(big, name):
    """k_posterior_stats (posterior_body<256, 1> + stats_body) against k_posterior
    (posterior_body<1024, 4>) and k_stats on the same features, labels and model: every posterior
    output bit for bit, the exactly summable statistics equal; both against the references."""
    case = pc.cases()[name]
    ref = pc.reference(case)
    labels = _labels_for(case)
    lab_case = pc.Case(case.name, case.model, case.feat, labels, None)
    e, n = big.eng, case.n
    big.set_model(case.model)
    load_rows(big, case.feat, labels, n)
    e.reset_window()
    e.posterior(True)
    e.accumulate_stats(None)
    a = outputs(big, n)
    e.post.fill_(-7.0)
    e.reset_window()
    e.posterior_and_stats(True)
    b = outputs(big, n)
    check_rows(case, ref, a["post"], a["pred"], a["conf"], a["evbits"])
    for key in ("post", "conf"):
        np.testing.assert_array_equal(_bits(a[key]), _bits(b[key]), err_msg=key)
    for key in ("pred", "evbits", "confusion"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    np.testing.assert_array_equal(a["confusion"], pc.reference_with(pc.device_model(case.model), lab_case).confusion)
    np.testing.assert_array_equal(_bits(a["count"]), _bits(b["count"]))
    np.testing.assert_array_equal(_bits(a["stats"][:16, :16]), _bits(b["stats"][:16, :16]))
    want, count = pc.stats_reference(lab_case)
    for got in (a, b):
        np.testing.assert_array_equal(got["count"], count)
        np.testing.assert_array_equal(got["stats"][:16, :16], want[:16, :16])
        check_rounded_blocks(got["stats"], want, n)


def check_rounded_blocks(got, want, n):
    """E^T X, X^T Y, X^T X: sums of n non-negative terms. 8 n 2^-52 bounds the rounding of such a
    sum in any order (n 2^-53 each for the device and the reference) with room for a few ulps
    between the device's log1p and the host's."""
    rtol = 8 * n * 2.0 ** -52
    for nm, blk in (("E^T X", np.s_[:16, 16:]), ("X^T Y", np.s_[16:, :16]), ("X^T X", np.s_[16:, 16:])):
        g, w = got[blk], want[blk]
        rel = np.abs(g - w)[w != 0] / w[w != 0]
        print(f"n {n} {nm}: max rel err {rel.max() if rel.size else 0.0:.3e} (bound {rtol:.3e})")
        np.testing.assert_allclose(g, w, rtol=rtol, atol=0, err_msg=nm)


@pytest.mark.parametrize("name", pc.stats_cases())
def test_weighted_statistics_match_the_reference(big, name):
    """k_stats with weights over one wave, two waves and a second block: count and E^T Y are sums
    of dyadic rationals and must be exact whatever the order of the atomics; E^T X, X^T Y and X^T X
    to the rounding of an n-term sum; unlabelled rows contribute to no block."""
    case = pc.cases()[name]
    want, count = pc.stats_reference(case)
    e, torch, n = big.eng, big.torch, case.n
    big.set_model(case.model)
    w = torch.zeros(big.group_cap, dtype=torch.float32, device=big.device)
    w[:n].copy_(torch.from_numpy(case.weights).to(big.device))
    load_rows(big, case.feat, case.labels, n)
    e.reset_window()
    e.accumulate_stats(w)
    out = outputs(big, n)
    np.testing.assert_array_equal(out["count"], count)
    np.testing.assert_array_equal(out["stats"][:16, :16], want[:16, :16])
    check_rounded_blocks(out["stats"], want, n)
    # the unlabelled rows with loud features and weights: nothing changes
    off = case.labels < 0
    feat = case.feat.copy()
    feat[off] = np.float32(1e6)
    w[:n][torch.from_numpy(off).to(big.device)] = 64.0
    load_rows(big, feat, case.labels, n)
    e.reset_window()
    e.accumulate_stats(w)
    out = outputs(big, n)
    np.testing.assert_array_equal(out["count"], count)
    np.testing.assert_array_equal(out["stats"][:16, :16], want[:16, :16])
    check_rounded_blocks(out["stats"], want, n)


# ---- refit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("name", ["zero-mass", "only-capped"])
def test_refit_with_inactive_domains_matches_the_host_model(pipe, name, pairs):
    """k_refit_nb through the shipped engine with min_count 1, ceil 0.95, the unknown floor and the
    capped unknown prior: a domain without labelled mass is inactive and so is every pair holding
    it; with only the capped domain active the cap does not apply."""
    rc = pc.refit_cases()[name]
    host = rc.host(pairs)
    seed = with_pairs(NaiveBayes.gpu(), rc.rho) if pairs else NaiveBayes.gpu()  # every column rewritten
    kw = rc.kwargs
    eng = pipe.eng
    eng.restore(rc.packed(), model_bytes(seed), 1)
    eng.set_p0(rc.p0().ravel())
    eng.set_refit(kw["alpha"], kw["prior_pseudo"], 1.0 / rc.temperature, kw["min_count"], pc.UNKNOWN, kw["ceil"])
    eng.refit_now()
    dev = np.frombuffer(np.asarray(eng.model_bytes(), dtype=np.uint8).tobytes(), dtype=MODEL_DTYPE)[0]
    ref = np.frombuffer(model_bytes(host).tobytes(), dtype=MODEL_DTYPE)[0]
    assert int(dev["n_pairs"]) == (len(host.pairs) if pairs else 0) and int(dev["mode"]) == 0
    for f in ("w", "bias") + (("w2", "bias2") if pairs else ()):
        np.testing.assert_allclose(dev[f], ref[f], rtol=1e-9, atol=1e-12, err_msg=f)
    live = np.isfinite(host.bias)  # an inactive domain's evidence mask is never read
    np.testing.assert_array_equal(dev["dom_mask"][:10][live], ref["dom_mask"][:10][live])
    np.testing.assert_array_equal(np.isneginf(dev["bias"][:10]), ~live)
    assert np.isneginf(dev["bias"][10:]).all()
    if name == "zero-mass":
        assert np.isneginf(dev["bias"][pc.ZERO_DOM]) and live.sum() == 9
    else:
        assert live.sum() == 1 and np.isfinite(dev["bias"][pc.UNKNOWN])
    if pairs:
        P = len(host.pairs)
        dead = ~np.isfinite(host.pair_b)
        if name == "zero-mass":
            np.testing.assert_array_equal(dead, (host.pairs == pc.ZERO_DOM).any(axis=1))
        else:
            assert dead.all()
        assert np.isneginf(dev["bias2"][:P][dead]).all() and not dev["w2"][:, :P][:, dead].any()
        assert np.isfinite(dev["bias2"][:P][~dead]).all()
    # the refitted image scores like the host model (inactive columns contribute nothing)
    f = pc.random_rows(41, 40)
    out = eng.score(f, None, None)
    np.testing.assert_allclose(out["post"][:, :10], host.posteriors(f.astype(np.float64)), rtol=1e-9, atol=1e-12)
    assert not out["post"][:, ~np.append(live, np.zeros(6, bool))].any()


def test_refit_nb_folds_add_in_the_same_launch(small):
    """Engine.refit_nb with n_dom = 8 and ``add``: the statistics become stats + add and the model is
    the refit of that sum, bit for bit; and it is NaiveBayes.learned over the first 8 domains."""
    torch, e = small.torch, small.eng
    a = pc.refit_cases()["zero-mass"]
    b = pc.RefitCase("add", pc.synthetic_stats(3, np.array([3, 0, 5, 2, 6, 1, 0, 9, 4, 2.0])), {}, 1.0, 0.0)
    A, B = a.packed(), b.packed()
    table = NaiveBayes.random_init_table(42)
    p0 = np.zeros((16, 16))
    p0[:, :10] = table
    p0_dev = torch.from_numpy(p0.ravel()).to(small.device)
    blank = NaiveBayes.learned(SufficientStats(), seed=42)
    images = []
    for acc, add in ((A.copy(), B), (A + B, None)):
        small.set_model(blank)
        acc_dev = torch.from_numpy(acc).to(small.device)
        add_dev = None if add is None else torch.from_numpy(add).to(small.device)
        e.refit_nb(acc_dev, p0_dev, 2.0, 1.0, 8, add_dev, -1)
        torch.cuda.synchronize(small.device)
        np.testing.assert_array_equal(_bits(acc_dev.cpu().numpy()), _bits(A + B))
        images.append(e.model.cpu().numpy().tobytes())
    assert images[0] == images[1]
    dev = np.frombuffer(images[0], dtype=MODEL_DTYPE)[0]
    doms = catalog.ALL_DOMAINS[:8]
    host = NaiveBayes.learned(a.stats.merge(b.stats), alpha=2.0, init=table[:, :8], domains=doms, prior_pseudo=1.0)
    ref = np.frombuffer(model_bytes(host).tobytes(), dtype=MODEL_DTYPE)[0]
    np.testing.assert_allclose(dev["w"], ref["w"], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(dev["bias"][:8], ref["bias"][:8], rtol=1e-13)
    assert np.isneginf(dev["bias"][8:]).all() and not dev["w"][:, 8:].any()
    np.testing.assert_array_equal(dev["dom_mask"], ref["dom_mask"])
