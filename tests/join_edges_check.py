"""Shared by tests/test_join_cases.py and tests/test_join_edges_gpu.py: the brute-force reference of
every join case (computed once per process) and the exact comparison of a KernelHarness run with it.

Run as a module (``python -m tests.join_edges_check CASE ...``) it is the child process of the probe
knob tests: MISLO_PROBE_* are read once per process, so each setting gets a fresh interpreter, which
runs the named cases through the harness and prints one JSON verdict line."""

import functools
import json
import sys

import numpy as np

from llm_slo_ebpf_toolkit_amd.collector import records
from llm_slo_ebpf_toolkit_amd.pipeline import join_cases, oracle

DEBUG_KEYS = ("candidates", "low_confidence", "fanout_dropped", "unmatched", "unsupported_type", "spans_enriched")
CAPS = dict(sig_cap=8192, span_cap=1024, group_cap=128)


@functools.lru_cache(maxsize=None)
def decoded(name: str, native: bool = False) -> oracle.Decoded:
    """The case's decoded rows; ``native``: connections folded to 32 bits as the window engine does."""
    d = oracle.decode_events(join_cases.cases()[name].events)
    if native:
        d.conn = records.conn32_np(d.conn).astype(np.uint64)
    return d


@functools.lru_cache(maxsize=None)
def reference(name: str, pi: int, native: bool = False) -> oracle.JoinResult:
    """``oracle.join_bruteforce`` of case ``name`` at its parameter set ``pi`` (shared, never modified)."""
    c = join_cases.cases()[name]
    spans = oracle.spans_native(c.spans) if native else c.spans
    return oracle.join_bruteforce(decoded(name, native), spans, c.n_groups, **c.params[pi])


@functools.lru_cache(maxsize=None)
def halo_reference(pi: int):
    """``ExchangeModel.join`` over ``join_cases.halo_pair()`` at parameter set ``pi``: per window the
    reference result, the rows joined [window rows | visible first-window rows] and the halo's size."""
    from llm_slo_ebpf_toolkit_amd.parallel.exchange import ExchangeModel

    xm = ExchangeModel(0, 1, join_cases.HALO_MS, 1024, 0, halo_windows=3)
    out = []
    for w in join_cases.halo_pair():
        d = oracle.decode_events(w.events)
        d.conn = records.conn32_np(d.conn).astype(np.uint64)
        halo = xm.halo()
        ref = xm.join(d, oracle.spans_native(w.spans), w.n_groups, **w.params[pi])
        out.append((ref, oracle.concat(d, halo), len(halo.ts)))
    return out


def kernel_ms_ref(attrs: np.ndarray) -> np.ndarray:
    """k_finalize's retrieval decomposition: dns + connect + tls (slots 0, 3, 5) added in that order in
    float32, absent slots skipped, NaN when the sum is not positive."""
    km = np.zeros(attrs.shape[0], dtype=np.float32)
    for slot in (0, 3, 5):
        v = attrs[:, slot]
        km = np.where(np.isnan(v), km, (km + v).astype(np.float32)).astype(np.float32)
    return np.where(km > 0, km, np.float32(np.nan)).astype(np.float32)


def harness_state(h, S: int, G: int) -> dict:
    e = h.eng
    return dict(
        top3=e.top3[: 3 * S].cpu().numpy().view(np.uint64).reshape(S, 3), cnt=e.cnt[:S].cpu().numpy(),
        attrs=e.attrs[:S].cpu().numpy(), conf=e.conf[:S].cpu().numpy(), kernel_ms=e.kernel_ms[:S].cpu().numpy(),
        gsum=e.gsum[:G].cpu().numpy(), gcnt=e.gcnt[:G].cpu().numpy())  # stripe 0 after the fold


def compare(tag: str, got: dict, feat: np.ndarray, debug: dict, ref: oracle.JoinResult, attrs=None, gsum=None,
            gcnt=None) -> None:
    """Exact, field by field; ``attrs`` / ``gsum`` / ``gcnt`` override the reference's (base_attrs runs)."""
    attrs = ref.attrs if attrs is None else attrs
    gsum = ref.gsum if gsum is None else gsum
    gcnt = ref.gcnt if gcnt is None else gcnt
    eq = np.testing.assert_array_equal
    eq(got["top3"], ref.top3, err_msg=f"{tag}: top3")
    eq(got["cnt"], ref.cnt, err_msg=f"{tag}: cnt")
    eq(got["attrs"], attrs, err_msg=f"{tag}: attrs")  # NaN == NaN at the same place
    eq(got["conf"], ref.conf, err_msg=f"{tag}: conf")
    eq(got["gsum"], gsum, err_msg=f"{tag}: gsum")
    eq(got["gcnt"], gcnt, err_msg=f"{tag}: gcnt")
    eq(feat, oracle.group_features(gsum, gcnt), err_msg=f"{tag}: feat")
    eq(got["kernel_ms"], kernel_ms_ref(attrs), err_msg=f"{tag}: kernel_ms")
    for k in DEBUG_KEYS:
        assert debug[k] == ref.debug[k], (tag, k, debug[k], ref.debug[k])


def run_case(h, name: str) -> int:
    """Every parameter set of one case through ``h.process``; returns the number of runs."""
    c = join_cases.cases()[name]
    S, G = len(c.spans), c.n_groups
    for pi, p in enumerate(c.params):
        h.set_join_params(**p)
        out = h.process(c.events, c.spans, G)
        ref = reference(name, pi)
        np.testing.assert_array_equal(out.feat, ref.feat, err_msg=f"{name} {p}: feat")
        compare(f"{name} {p}", harness_state(h, S, G), out.feat, out.debug, ref)
    return len(c.params)


def make_harness():
    from llm_slo_ebpf_toolkit_amd.models.bayes import NaiveBayes
    from llm_slo_ebpf_toolkit_amd.ops.engine import KernelHarness

    h = KernelHarness(**CAPS)
    h.set_model(NaiveBayes.ref())
    return h


def main(argv) -> int:
    import os

    verdict = {"ok": False, "runs": 0, "failed": None,
               "knobs": {k: v for k, v in os.environ.items() if k.startswith("MISLO_PROBE_")}}
    try:
        h = make_harness()
        for name in argv:
            verdict["runs"] += run_case(h, name)
        verdict["ok"] = True
    except AssertionError as e:  # a mismatch: report it, the parent fails the test
        verdict["failed"] = str(e)[:2000]
    print(json.dumps(verdict), flush=True)
    return 0 if verdict["ok"] else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
