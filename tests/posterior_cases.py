"""Crafted rows for the K3 kernels (ops/csrc/posterior.hip: posterior, statistics, refit) and their
float64 references. Plain numpy: no GPU code is imported here.

A case is a named bundle -- a model, float32 features [n, 16], optional label codes, weights and
application counts. tests/test_posterior_cases.py proves on the CPU that the cases deserve the
assertions tests/test_posterior_gpu.py makes about them (top-2 gaps, exactly summable label masses,
rows on both sides of every threshold).

* The posterior reference is models/bayes.py (posteriors / predict / evidence_bits /
  AppEvidence.state) evaluated on ``model_from_bytes(model_bytes(m))``: the thresholds are then the
  float32 values the device reads.
* The statistics reference is U^T V, U = [E | X], V = [Y | X], over the labelled rows only, written
  out in float64 numpy: Y = soft_labels(code) * weight over 16 columns, X = log1p(max(nan -> NOMINAL,
  0)); X^T X and E^T X are unweighted, as in the kernel. SufficientStats.add has no E^T X and cannot
  take label < 0, so it is not used.
"""

from __future__ import annotations

import functools
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from llm_slo_ebpf_toolkit_amd.models.bayes import (LDA, NOMINAL, AppEvidence, LinearPosteriorModel, NaiveBayes,
                                                   SufficientStats, label_code, marginalize, samples_to_arrays,
                                                   soft_labels, with_pairs)
from llm_slo_ebpf_toolkit_amd.models.sample import load_samples_jsonl
from llm_slo_ebpf_toolkit_amd.ops.engine import model_bytes, model_from_bytes
from llm_slo_ebpf_toolkit_amd.signals import catalog

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "ref_multi_fault_samples.jsonl")
ROW_COUNTS = (1, 15, 16, 17, 63, 64, 65, 129)   # row-group and block edges of k_posterior (16 / 64 rows)
STATS_ROWS = (3, 257, 1030)                     # one wave; two waves; a second block of k_stats
MIN_GAP = 1e-6                                  # top-2 gap a compared ``pred`` needs in the reference
UNKNOWN = catalog.DOMAIN_INDEX["unknown"]
THR32 = np.array([s.elevated for s in catalog.SIGNALS], dtype=np.float32)
APP_THR_MS = 100.0
# slots the marginalised threshold case cannot observe (dropping slot 4 would leave provider_throttle
# and provider_error mirror images of each other: structural near-ties in the reference)
DROPPED_SLOTS = (2, 7, 12, 15)


@dataclass
class Case:
    name: str
    model: LinearPosteriorModel
    feat: np.ndarray                       # float32 [n, 16]
    labels: Optional[np.ndarray] = None    # int32 label codes (models/bayes.py label_code), -1 = unlabelled
    weights: Optional[np.ndarray] = None   # float32 [n]
    app_cnt: Optional[np.ndarray] = None   # uint32 [n, 2] (spans, retrieval sum in 10 us units)
    tie: bool = False                      # every row's two best logits are bitwise equal

    @property
    def n(self) -> int:
        return len(self.feat)


@dataclass
class Reference:
    post: np.ndarray                       # [n, 10]
    pred: np.ndarray                       # [n]
    evbits: np.ndarray                     # [n, 10] uint32
    gap: np.ndarray                        # [n] top-2 gap: logits (single-fault) or marginals (pairs)
    state: Optional[np.ndarray]            # [n] application evidence state, or None
    confusion: Optional[np.ndarray]        # [16, 16] int64, or None without labels


def device_model(m: LinearPosteriorModel) -> LinearPosteriorModel:
    """The host model the device image of ``m`` evaluates (float32 thresholds), with m's application
    evidence (an image of its own on the device, in float64)."""
    d = model_from_bytes(model_bytes(m))
    d.app = m.app
    return d


def reference_with(m: LinearPosteriorModel, case: Case) -> Reference:
    v = case.feat.astype(np.float64)
    st = m.app.state(case.app_cnt, case.feat) if (m.app is not None and case.app_cnt is not None) else None
    with np.errstate(invalid="ignore", over="ignore"):
        post = m.posteriors(v, st)
        pred = m.predict(v, st)
        score = m.logits(v, st) if m.pairs is None else post
    top = np.sort(score, axis=1)
    with np.errstate(invalid="ignore"):
        gap = top[:, -1] - top[:, -2]
    conf = None
    if case.labels is not None:
        y = case.labels.astype(np.int64)
        ok = (y >= 0) & ((y & 0xFF) < 16)
        conf = np.zeros((16, 16), dtype=np.int64)
        np.add.at(conf, ((y & 0xFF)[ok], pred[ok]), 1)
    return Reference(post, pred.astype(np.int64), m.evidence_bits(v, st), gap, st, conf)


def reference(case: Case) -> Reference:
    """The float64 reference of a case, computed once per case name."""
    return _cached_reference(case.name)


@functools.lru_cache(maxsize=None)
def _cached_reference(name: str) -> Reference:
    case = cases()[name]
    return reference_with(device_model(case.model), case)


def reference_unrounded(case: Case) -> Reference:
    """The same on the model as built (float64 thresholds): the MODEL_DTYPE round trip check."""
    return reference_with(case.model, case)


def stats_reference(case: Case) -> Tuple[np.ndarray, np.ndarray]:
    """(U^T V [32, 32], count [16]) over the labelled rows of a statistics case."""
    m = device_model(case.model)
    on = case.labels >= 0
    v = case.feat.astype(np.float64)[on]
    w = np.ones(on.sum()) if case.weights is None else case.weights.astype(np.float64)[on]
    Y = soft_labels(case.labels[on], 16) * w[:, None]
    E = ((v >= m.thresholds[None, :]) & ~np.isnan(v)).astype(np.float64)
    X = np.log1p(np.maximum(np.where(np.isnan(v), NOMINAL[None, :], v), 0.0))
    U, V = np.concatenate([E, X], axis=1), np.concatenate([Y, X], axis=1)
    return U.T @ V, Y.sum(axis=0)


# ---- builders ---------------------------------------------------------------------------------
def random_rows(seed: int, n: int, hi=None, nan: float = 0.3) -> np.ndarray:
    """[n, 16] float32: uniform in [0, hi) per slot (default three times the slot's threshold, so a
    present signal is elevated two times in three), ``nan`` of the entries absent."""
    rng = np.random.default_rng(seed)
    hi = 3.0 * THR32.astype(np.float64) if hi is None else np.broadcast_to(np.float64(hi), (16,))
    f = (rng.random((n, 16)) * hi[None, :]).astype(np.float32)
    f[rng.random((n, 16)) < nan] = np.nan
    return f


def pairs_trimmed(m: LinearPosteriorModel, keep: int) -> LinearPosteriorModel:
    """A 2-fault model with only its first ``keep`` pair hypotheses (one MFMA pair tile for <= 16)."""
    out = LinearPosteriorModel(m.name, m.weights.copy(), m.bias.copy(), m.evidence_mask.copy(), m.feature_mode,
                               m.thresholds.copy(), None, None if m.table_mask is None else m.table_mask.copy())
    out.pair_w, out.pair_b = m.pair_w[:, :keep].copy(), m.pair_b[:keep].copy()
    out.pairs, out.pair_rho, out.app = m.pairs[:keep].copy(), m.pair_rho, m.app
    return out


def fixture_rows() -> Tuple[np.ndarray, np.ndarray]:
    vals, labels = samples_to_arrays(load_samples_jsonl(FIXTURE))
    return vals.astype(np.float32), labels


def lda_model() -> LinearPosteriorModel:
    vals, labels = fixture_rows()
    st = SufficientStats()
    st.add(vals.astype(np.float64), labels)
    return LDA.fit(st)


def _threshold_rows(seed: int) -> np.ndarray:
    """For every slot: the threshold, its float32 neighbours, +-inf, -0.0, a negative value and a
    subnormal in that slot of an otherwise random row; then an all-NaN row. 16 * 8 + 1 = 129 rows."""
    f = random_rows(seed, 16 * 8 + 1)
    for s in range(16):
        t = THR32[s]
        edge = [t, np.nextafter(t, np.float32(-np.inf)), np.nextafter(t, np.float32(np.inf)), np.float32(np.inf),
                np.float32(-np.inf), np.float32(-0.0), np.float32(-7.5), np.float32(1e-42)]
        f[8 * s:8 * s + 8, s] = np.array(edge, dtype=np.float32)
    f[-1, :] = np.nan
    return f


def dyadic_model(scale: float = 64.0) -> LinearPosteriorModel:
    """NaiveBayes.gpu() with every weight and bias rounded to a multiple of 1 / ``scale``: a binary
    row's logits are then exact sums in any order, on the host (BLAS) and on the device (MFMA)."""
    g = NaiveBayes.gpu()
    return LinearPosteriorModel("dyadic", np.round(g.weights * scale) / scale, np.round(g.bias * scale) / scale,
                                g.evidence_mask.copy(), "binary", g.thresholds.copy(), None, g.table_mask.copy())


TIE_LOW, TIE_HIGH = 3, 6


def tie_model() -> LinearPosteriorModel:
    """Two domain columns are copies (TIE_LOW takes TIE_HIGH's weights and bias; the lower index is
    neither lane 0 nor the column the values came from) and lead every row by a raised bias: the
    reference logits of the two are bitwise equal, and the documented winner is the lower index."""
    m = dyadic_model()
    m.bias[TIE_HIGH] += 16.0
    m.weights[:, TIE_LOW] = m.weights[:, TIE_HIGH]
    m.bias[TIE_LOW] = m.bias[TIE_HIGH]
    m.evidence_mask[:, TIE_LOW] = m.evidence_mask[:, TIE_HIGH]
    return m


def single_active_model(keep: int = 5) -> LinearPosteriorModel:
    m = NaiveBayes.gpu()
    b = np.full_like(m.bias, -np.inf)
    b[keep] = m.bias[keep]
    m.bias = b
    return m


def underflow_model(scale: float = 8192.0) -> LinearPosteriorModel:
    """Logits so far apart (the expert table's, times ``scale``) that every loser's exp is 0."""
    m = NaiveBayes.gpu()
    m.weights = m.weights * scale
    m.bias = m.bias * scale
    return m


def label_codes(seed: int, n: int, sets: bool = True) -> np.ndarray:
    """Primary labels 0..9, a third of the rows unlabelled (-1), label sets of size 1, 2 or 4 (soft
    labels), and one code whose primary is >= 16."""
    rng = np.random.default_rng(seed)
    out = np.empty(n, dtype=np.int32)
    for r in range(n):
        p = int(rng.integers(0, 10))
        if r % 3 == 2:
            out[r] = -1
            continue
        size = (1, 2, 4)[int(rng.integers(0, 3))] if sets else 1
        others = [d for d in rng.permutation(10).tolist() if d != p][:size - 1]
        out[r] = label_code(p, [p] + others)
    if n > 4:
        out[4] = label_code(20)
    return out


def _app_case(name: str, model: LinearPosteriorModel) -> Case:
    """20 rows, two 16-row groups: rows with and without application counts interleaved; residuals
    exactly at the threshold, one 10 us unit below it, well above; NaN in each of slots 0 / 3 / 5."""
    n = 20
    f = random_rows(91, n)
    cnt = np.zeros((n, 2), dtype=np.uint32)
    thr_units = int(APP_THR_MS * 100)
    shares = [(10.0, np.nan, 5.0), (np.nan, 20.0, 5.0), (10.0, 20.0, np.nan), (np.nan, np.nan, np.nan),
              (12.5, 30.25, 7.0)]
    for r in range(n):
        a, b, c = shares[r % len(shares)]
        f[r, 0], f[r, 3], f[r, 5] = a, b, c
        kern_units = int(round(sum(x for x in (a, b, c) if x == x) * 100))  # the shares are multiples of 10 us
        kind = r % 4
        if kind == 0:
            continue                                  # absent: n == 0
        spans = 1 if r % 8 < 4 else 4                 # a mean over 4 spans: the sum is 4 x as large
        delta = {1: 0, 2: -1, 3: 2500 * spans}[kind]  # at the threshold / one unit below / 25 ms above
        cnt[r] = (spans, spans * (thr_units + kern_units) + delta)
    m = model
    m.app = AppEvidence.expert(APP_THR_MS)
    return Case(name, m, f, None, None, cnt)


def _stats_case(n: int) -> Case:
    f = random_rows(300 + n, n, hi=300.0)
    rng = np.random.default_rng(7 + n)
    f[rng.random((n, 16)) < 0.05] = 0.0
    f[rng.random((n, 16)) < 0.05] = np.float32(-3.25)
    w = rng.choice(np.array([0.25, 0.5, 1.0, 2.0], dtype=np.float32), size=n)
    return Case(f"stats-{n}", NaiveBayes.gpu(), f, label_codes(11 + n, n), w)


@functools.lru_cache(maxsize=None)
def cases() -> Dict[str, Case]:
    out: List[Case] = []
    pairs36 = with_pairs(NaiveBayes.gpu(), 0.2)
    kinds = {"ref": NaiveBayes.ref(), "gpu": NaiveBayes.gpu(), "pairs36": pairs36, "pairs16": pairs_trimmed(pairs36, 16)}
    for k, (kind, m) in enumerate(kinds.items()):
        for n in ROW_COUNTS:
            out.append(Case(f"rows-{kind}-{n}", m, random_rows(1000 * k + n, n)))
    lda = lda_model()
    out.append(Case("lda-fixture", lda, fixture_rows()[0]))
    f = random_rows(77, 129, hi=300.0)
    rng = np.random.default_rng(78)
    f[rng.random(f.shape) < 0.05] = 0.0
    f[rng.random(f.shape) < 0.05] = np.float32(-12.0)
    f[rng.random(f.shape) < 0.02] = np.float32(-0.0)
    out.append(Case("lda-random", lda, f))
    out.append(Case("thr-gpu", NaiveBayes.gpu(), _threshold_rows(5)))
    seen = [s.name for s in catalog.SIGNALS if s.slot not in DROPPED_SLOTS]
    out.append(Case("thr-marginalized", marginalize(NaiveBayes.gpu(), seen), _threshold_rows(6)))
    out.append(Case("tie", tie_model(), random_rows(21, 70), tie=True))
    out.append(Case("single-active", single_active_model(), random_rows(22, 33)))
    out.append(Case("underflow", underflow_model(), random_rows(28, 33)))
    out.append(Case("labels", NaiveBayes.gpu(), random_rows(24, 70), label_codes(25, 70)))
    out.append(_app_case("app-single", NaiveBayes.gpu()))
    out.append(_app_case("app-pairs", with_pairs(NaiveBayes.gpu(), 0.2)))
    out.extend(_stats_case(n) for n in STATS_ROWS)
    return {c.name: c for c in out}


def score_cases() -> List[str]:
    """Names of the cases scored through the posterior kernel."""
    return [n for n in cases() if not n.startswith("stats-")]


def stats_cases() -> List[str]:
    return [f"stats-{n}" for n in STATS_ROWS]


# ---- refit ------------------------------------------------------------------------------------
ZERO_DOM = catalog.DOMAIN_INDEX["provider_throttle"]   # the domain without labelled mass


@dataclass
class RefitCase:
    name: str
    stats: SufficientStats
    kwargs: Dict[str, object]      # NaiveBayes.learned's (without temperature)
    temperature: float
    rho: float                     # pair prior mass (with_pairs) where the case is run with pairs

    def packed(self) -> np.ndarray:
        """f64[1040]: the device's statistics layout ([32 x 32] U^T V, then count[16])."""
        S = np.zeros((32, 32))
        S[:16, :10] = self.stats.elevated_sum
        S[16:, :10] = self.stats.x_sum
        S[16:, 16:] = self.stats.xx
        out = np.zeros(1040)
        out[:1024] = S.ravel()
        out[1024:1034] = self.stats.count
        return out

    def p0(self) -> np.ndarray:
        """[2, 16, 16] f64: the Beta prior's table and the likelihood floor, as the device reads them."""
        p = np.zeros((2, 16, 16))
        init = self.kwargs.get("init")
        p[0, :, :10] = init if init is not None else NaiveBayes.random_init_table(int(self.kwargs.get("seed", 42)))
        if self.kwargs.get("floor") is not None:
            p[1, :, :10] = self.kwargs["floor"]
        return p

    def host(self, pairs: bool) -> LinearPosteriorModel:
        m = NaiveBayes.learned(self.stats, temperature=self.temperature, **self.kwargs)
        return with_pairs(m, self.rho, self.temperature) if pairs else m


def synthetic_stats(seed: int, count: np.ndarray) -> SufficientStats:
    rng = np.random.default_rng(seed)
    st = SufficientStats()
    st.count = np.asarray(count, dtype=np.float64)
    st.elevated_sum = np.floor(rng.random((16, 10)) * (st.count[None, :] + 1.0)).clip(0.0, st.count[None, :])
    return st


@functools.lru_cache(maxsize=None)
def refit_cases() -> Dict[str, RefitCase]:
    kw = {"alpha": 2.0, "seed": 42, "prior_pseudo": 1.0, "min_count": 1.0, "init": None,
          "floor": NaiveBayes.unknown_floor(), "cap_domain": "unknown", "ceil": 0.95}
    count = np.array([12, 7, 9, 5, 0, 11, 6, 40, 3, 8], dtype=np.float64)
    assert count[ZERO_DOM] == 0 and count[UNKNOWN] == count.max()
    only = np.zeros(10)
    only[UNKNOWN] = 23.0
    out = [RefitCase("zero-mass", synthetic_stats(1, count), dict(kw), 2.5, 0.3),
           RefitCase("only-capped", synthetic_stats(2, only), dict(kw), 2.5, 0.3)]
    return {c.name: c for c in out}
