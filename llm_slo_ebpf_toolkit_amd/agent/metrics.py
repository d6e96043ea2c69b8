"""Agent Prometheus surface: every REF metric name/type/label set (REF cmd/agent/main.go:137-302,
SURVEY §2.8) plus the GPU window engine's metrics (additive, ``llm_slo_agent_gpu_*``).

GPU histograms arrive as per-window bucket counts from the decode kernel (LDS-privatised,
RCCL all-reduced across GPUs); ``observe_window_hist`` folds them into Prometheus
histograms without re-observing events. The kernel's buckets are ``le`` buckets
(v in (edge[b-1], edge[b]]) over the catalogue edges, of which REF's DNS edges
{1..800} are a prefix, so the REF-named DNS histogram keeps exact ``le`` semantics.
"""

from __future__ import annotations

import os
import time
from typing import Iterable, Sequence

import numpy as np

from ..contracts.types import ProbeEventV1
from ..export.prometheus import Registry
from ..signals import catalog

EVENT_KINDS = ("slo", "probe", "both")
DROP_REASONS = ("rate_limit", "schema", "emit", "xchg_cap", "import_cap")


def _nz(v: str, fallback: str) -> str:
    v = (v or "").strip()
    return v if v else fallback


class AgentMetrics:
    def __init__(self, event_kind: str, capability_mode: str, supported: Sequence[str], enabled: Sequence[str]):
        r = self.registry = Registry()
        self.heartbeat = r.gauge("llm_slo_agent_heartbeat", "Unix timestamp of latest emitted sample.")
        self.up = r.gauge("llm_slo_agent_up", "Agent process liveness.")
        self.cpu = r.gauge("llm_slo_agent_cpu_overhead_pct", "Estimated agent CPU overhead percentage.")
        self.kind = r.gauge("llm_slo_agent_event_kind", "Selected event-kind mode (one-hot gauge).", ("kind",))
        self.mode = r.gauge("llm_slo_agent_capability_mode", "Detected capability mode (one-hot gauge).", ("mode",))
        self.sig_enabled = r.gauge("llm_slo_agent_signal_enabled", "Signal enablement toggle by signal name.",
                                   ("signal",))
        self.dropped = r.counter("llm_slo_agent_dropped_events_total", "Dropped probe events by reason.", ("reason",))
        self.hello = r.counter("llm_ebpf_hello_syscalls_total", "Hello tracer syscall events by comm.",
                               ("node", "pod", "comm"))
        self.dns = r.histogram("llm_ebpf_dns_latency_ms", "DNS latency observed from probe events.",
                               catalog.REF_DNS_BUCKETS, ("node", "pod", "namespace"))
        self.probe_events = r.counter("llm_ebpf_probe_events_total", "Probe events observed by signal and status.",
                                      ("signal", "status"))
        # ---- GPU window engine (additive) ----
        self.win_events = r.counter("llm_slo_agent_gpu_window_events_total", "Events processed by the GPU engine.")
        self.win_total = r.counter("llm_slo_agent_gpu_windows_total", "Windows processed by the GPU engine.")
        self.win_latency = r.histogram("llm_slo_agent_gpu_window_latency_ms",
                                       "Ring drain to attribution latency per window.",
                                       (0.5, 1, 2, 5, 10, 20, 50, 100, 200, 500, 1000))
        self.attr = r.counter("llm_slo_agent_attributions_total", "Incident attributions by predicted domain.",
                              ("domain",))
        self.scored = r.counter("llm_slo_agent_incidents_scored_total",
                                "Incident groups scored per window by top domain, and whether an attribution was "
                                "emitted (only groups with SLO impact are).", ("domain", "emitted"))
        self.corr = r.counter("llm_slo_agent_correlation_pairs_total",
                              "Span/signal correlation outcomes (REF DebugStats) from the join kernel.", ("outcome",))
        self.ring_dropped = r.gauge("llm_slo_agent_ring_dropped_events", "Events dropped by full producer rings.")
        self.ring_defs = r.counter("llm_slo_agent_ring_definitions_total",
                                   "Context / trace id definition records consumed from the BPF ring.")
        self.ring_busy = r.counter("llm_slo_agent_ring_busy_stops_total",
                                   "Windows whose ring consumption stopped at a record still being written.")
        self.ring_backlog = r.gauge("llm_slo_agent_ring_backlog_bytes", "Unconsumed bytes in the BPF ring buffer.")
        self.flush_loaded = r.gauge("llm_slo_agent_flush_program_loaded",
                                    "1 when the cut's per-CPU flush program (mislo_flush) is pinned and run.")
        self.flush_errors = r.gauge("llm_slo_agent_flush_errors",
                                    "Per-CPU flush runs that failed (other than offline CPUs), since start.")
        self.host_us = r.gauge("llm_slo_agent_window_host_us", "Host time to assemble the last window (us).")
        self.windows_skipped = r.counter("llm_slo_agent_windows_skipped_total",
                                         "Window cuts skipped after the loop stalled for more than a window period.")
        self.workers = r.gauge("llm_slo_agent_window_workers", "Window workers (GPUs) the agent is running.")
        self.worker_restarts = r.counter("llm_slo_agent_worker_restarts_total",
                                         "Worker pool restarts after a worker died (the survivors' GPUs go on).")
        self.rss = r.gauge("llm_slo_agent_memory_rss_bytes", "Agent process resident set size (bytes).")
        self.otlp = r.gauge("llm_slo_agent_otlp_spans", "OTLP receiver span records since start by outcome: accepted "
                            "into the span ring, dropped (ring full), rejected (malformed export), conflict (a pod "
                            "bound to another service), spoofed (a pod named from another pod's address), "
                            "first_token_late (a first-token record after its request span, which counted it).",
                            ("outcome",))
        self.cg_mem = r.gauge("llm_slo_agent_memory_cgroup_bytes",
                              "Memory charged to the agent's cgroup (v2 memory.current, v1 usage_in_bytes): what a "
                              "pod memory limit is enforced on, next to RSS.")
        self.burn_err = r.gauge("llm_slo_agent_burn_rate_prediction_error",
                                "Mean relative error of the scored SLO burn-rate forecasts.")
        # the open-request tracker (agent --deadline-breach, pipeline/openreq.py)
        self.deadline_breaches = r.counter("llm_slo_agent_deadline_breaches_total",
                                           "TTFT breaches counted when the request's deadline passed with no first "
                                           "token (start records, --deadline-breach), by service.", ("service",))
        self.open_requests = r.gauge("llm_slo_agent_open_requests",
                                     "Rows of the open-request table by state: open (started, no first token), "
                                     "counted (breach counted at its deadline, not reported yet), resolved (an "
                                     "SLI that came ahead of its start record).", ("state",))
        self.open_events = r.counter("llm_slo_agent_open_request_events_total",
                                     "Open-request table events: dup_start, start_after_sli, dropped_full, expired "
                                     "(counted, never reported within the ttl), false_deadline (counted, then "
                                     "reported within the SLO).", ("reason",))
        # the TTFT sketch (agent --ttft-distribution, pipeline/slisketch.py): every service's TTFT as
        # the agent sees it. The name keeps it apart from the demo service's own llm_slo_ttft_ms.
        from ..pipeline import slisketch as sk

        self.ttft_hist = r.histogram("llm_slo_agent_ttft_ms",
                                     "TTFT (ms) of the SLI records the agent counted, by service, at the "
                                     "llm_slo_ttft_ms boundaries (exact counts and sum, built on the GPU).",
                                     sk.EDGES, ("service",))
        self.ttft_quantile = r.gauge("llm_slo_agent_ttft_quantile_ms",
                                     "TTFT quantile (ms) by service from the GPU sketch (16 buckets per octave: "
                                     "within 1/32 of the nearest-rank value); scope window = the last window, "
                                     "rolling = the last --ttft-horizon-windows windows.",
                                     ("service", "quantile", "scope"))
        self.ttft_events = r.counter("llm_slo_agent_ttft_sketch_events_total",
                                     "TTFT sketch events: invalid (a counted record with a NaN or negative TTFT, in "
                                     "no bucket), underflow (below 0.125 ms), overflow (2^21 ms or more).",
                                     ("reason",))
        # request exemplars (agent --request-exemplars, pipeline/exemplars.py): the exact maximum, which
        # the sketch's buckets cannot give. Plain series: no OpenMetrics exemplar syntax
        self.ttft_max = r.gauge("llm_slo_agent_ttft_max_ms",
                                "Largest TTFT (ms) of the last window by service: the first request exemplar, "
                                "chosen on the GPU (exact).", ("service",))
        self.exemplar_events = r.counter("llm_slo_agent_exemplar_events_total",
                                         "Request-exemplar events: invalid (a counted record with a NaN or negative "
                                         "TTFT), out_of_group (an SLI record of a group beyond the window's).",
                                         ("reason",))
        # pod breakdown (agent --pod-breakdown, pipeline/podrank.py), over the recent windows. No per-pod
        # label series: the label set would churn with every rollout
        self.pods_seen = r.gauge("llm_slo_agent_pods_seen",
                                 "Distinct pods with a counted request over the recent windows, by service.", ("service",))
        self.pods_breaching = r.gauge("llm_slo_agent_pods_breaching",
                                      "Distinct pods with at least one TTFT breach over the recent windows, by service.",
                                      ("service",))
        self.top_pod_share = r.gauge("llm_slo_agent_breach_top_pod_share",
                                     "Share of the service's recent TTFT breaches on its worst pod (0 without a "
                                     "breach): near 1 = one replica, near 1/pods = service-wide.", ("service",))
        self.pod_events = r.counter("llm_slo_agent_pod_breakdown_events_total",
                                    "Pod-breakdown events: invalid (a counted record with a NaN or negative TTFT), "
                                    "out_of_group (an SLI record of a group beyond the window's), pod_out_of_range (a "
                                    "pod id of 2^20 or more, in no pod row), pair_overflow (a record whose (service, "
                                    "pod) pair found no place among the window's --pod-pairs).", ("reason",))
        # breach onset (agent --breach-onset, pipeline/onset.py): when the current run of breaches began
        self.onset_age = r.gauge("llm_slo_agent_breach_onset_age_seconds",
                                 "Seconds from the onset of the service's current TTFT breach excursion (CUSUM over "
                                 "time bins of the requests' start times, on the GPU) to the window's cut; 0 when quiet.",
                                 ("service",))
        self.onset_state = r.gauge("llm_slo_agent_breach_onset_state",
                                   "Breach-onset state by service: 0 quiet, 1 excursion, 2 alarm (the excursion has "
                                   "reached --onset-alarm-breaches over the reference rate).", ("service",))
        self.onset_events = r.counter("llm_slo_agent_breach_onset_events_total",
                                      "Breach-onset events: invalid (a counted record with a NaN or negative TTFT), "
                                      "out_of_group (an SLI record of a group beyond the window's), no_time (no start "
                                      "time, in no bin), future (a start time past the cut, placed in the newest bin), "
                                      "too_old (a start time before the ring, placed nowhere).", ("reason",))
        # decode SLI (agent --decode-sli, pipeline/decodesli.py): time per output token and goodput
        self.tpot_quantile = r.gauge("llm_slo_agent_tpot_ms",
                                     "Time per output token quantile (ms) by service over the last "
                                     "--decode-horizon-windows windows, from the histogram on the GPU (16 buckets per "
                                     "octave: within 1/32 of the nearest-rank value).", ("service", "quantile"))
        self.goodput = r.gauge("llm_slo_agent_goodput_ratio",
                               "Share of the service's finished requests over the last --decode-horizon-windows windows "
                               "that met both the TTFT and the TPOT SLO.", ("service",))
        self.decode_requests = r.counter("llm_slo_agent_decode_requests_total",
                                         "Finished requests with a TPOT, by service and outcome: good (both SLOs met), "
                                         "ttft_only / tpot_only (that SLO breached alone), both.", ("service", "outcome"))
        self.decode_events = r.counter("llm_slo_agent_decode_events_total",
                                       "Decode SLI events: invalid (a TPOT with a NaN or negative TTFT), out_of_group (a "
                                       "group beyond the window's), no_decode (a finished request without a TPOT).",
                                       ("reason",))
        # TTFT drift (agent --ttft-drift, pipeline/drift.py): recent against baseline
        self.drift_state = r.gauge("llm_slo_agent_ttft_drift_state",
                                   "TTFT drift of the service: 0 calm, 1 slow (the recent windows are significantly and "
                                   "materially slower than the baseline), 2 fast, 3 warming (too few records or baseline "
                                   "windows; also the window of a rebase).", ("service",))
        self.drift_distance = r.gauge("llm_slo_agent_ttft_drift_distance",
                                      "One-sided two-sample Kolmogorov-Smirnov distance of the service's recent TTFT "
                                      "distribution towards slower than its baseline, 0..1.", ("service",))
        self.drift_ratio = r.gauge("llm_slo_agent_ttft_drift_shift_ratio",
                                   "Recent p50 TTFT over the baseline's p50, by service.", ("service",))
        self.drift_events = r.counter("llm_slo_agent_ttft_drift_events_total",
                                      "TTFT drift events: invalid (ttft NaN or negative), out_of_group (a group beyond the "
                                      "window's), admitted / withheld (a window leaving the gap entered the baseline / was "
                                      "kept out while the service was slow), rebased (a baseline dropped after hold_max "
                                      "slow windows).", ("reason",))
        # error SLI (agent --error-sli, pipeline/errsli.py): outcome classes and budget burn
        self.outcomes = r.counter("llm_slo_agent_request_outcomes_total",
                                  "Finished requests by service and outcome class: ok, client, cancelled, throttled, "
                                  "timeout, unavailable, server, other.", ("service", "outcome"))
        self.error_ratio = r.gauge("llm_slo_agent_error_ratio",
                                   "Share of the service's finished requests over the last --error-horizon-windows "
                                   "windows whose class counts against the availability budget.", ("service",))
        self.error_burn = r.gauge("llm_slo_agent_error_burn_rate",
                                  "Availability budget multiples the service spends over a burn-rate pair's long or "
                                  "short window.", ("service", "pair", "window"))
        self.error_firing = r.gauge("llm_slo_agent_error_burn_firing",
                                    "1 while both windows of the burn-rate pair burn at its factor or more.",
                                    ("service", "pair"))
        self.error_events = r.counter("llm_slo_agent_error_events_total",
                                      "Error SLI events: out_of_group (a group beyond the window's), reserved (an "
                                      "outcome class of 8-15, which nothing writes).", ("reason",))
        # load SLI (agent --load-sli, pipeline/loadsli.py): traffic and saturation
        self.load_state = r.gauge("llm_slo_agent_load_state",
                                  "Load state by service: 0 steady, 1 surge (arrivals up by --load-factor), 2 slowdown "
                                  "(concurrency up at the same arrivals), 3 drop (arrivals down), 4 warming.", ("service",))
        self.request_rate = r.gauge("llm_slo_agent_request_rate",
                                    "Requests per second arriving at the service over the recent range and over the "
                                    "base range before it.", ("service", "range"))
        self.concurrency = r.gauge("llm_slo_agent_concurrency",
                                   "Requests in flight at the service, averaged over the recent and the base range, and "
                                   "the ring's peak.", ("service", "range"))
        # saturation curve (agent --saturation-curve, pipeline/satcurve.py): how much load fits the TTFT SLO
        self.saturation_state = r.gauge("llm_slo_agent_saturation_state",
                                        "Saturation state by service: 0 unknown, 1 no_knee (no concurrency level over the "
                                        "TTFT SLO's error budget), 2 below the knee, 3 saturated (recent concurrency at or "
                                        "above the knee).", ("service",))
        self.saturation_knee = r.gauge("llm_slo_agent_saturation_knee_concurrency",
                                       "The concurrency above which the service exceeds its TTFT SLO's error budget (the last "
                                       "valid knee).", ("service",))
        self.saturation_headroom = r.gauge("llm_slo_agent_saturation_headroom_ratio",
                                           "Knee concurrency over recent concurrency (the last values with a knee).",
                                           ("service",))
        self.saturation_events = r.counter("llm_slo_agent_saturation_events_total",
                                           "Saturation curve events: out_of_group, invalid (a duration NaN, negative or above "
                                           "a day), no_time, future, too_old, clipped (started before the ring: not in the "
                                           "curve), no_ttft (occupies its interval, not in the curve).", ("reason",))
        # TTFT phase split (agent --retrieval-sli, pipeline/retrsli.py): retrieval against model time
        self.retrieval_quantile = r.gauge("llm_slo_agent_retrieval_ms",
                                          "Retrieval time quantile (ms) by service over the last "
                                          "--retrieval-horizon-windows windows, of the requests that report a breakdown, "
                                          "from the histogram on the GPU (within 1/32 of the nearest-rank value).",
                                          ("service", "quantile"))
        self.model_ttft_quantile = r.gauge("llm_slo_agent_model_ttft_ms",
                                           "Model time quantile (ms), TTFT minus retrieval, by service over the last "
                                           "--retrieval-horizon-windows windows.", ("service", "quantile"))
        self.retrieval_share = r.gauge("llm_slo_agent_retrieval_share",
                                       "Retrieval time over TTFT, summed over the service's requests with a breakdown in "
                                       "the last --retrieval-horizon-windows windows.", ("service",))
        self.ttft_phase_state = r.gauge("llm_slo_agent_ttft_phase_state",
                                        "Which phase the service's TTFT breaches come from over the horizon: 0 unknown, 1 ok "
                                        "(within the error budget), 2 retrieval_bound, 3 model_bound, 4 mixed.", ("service",))
        self.ttft_breach_phase = r.counter("llm_slo_agent_ttft_breach_phase_total",
                                           "Requests with a retrieval breakdown by service and TTFT-breach phase: ok, "
                                           "ok_slow_retrieval, model, model_slow_retrieval, retrieval, combined.",
                                           ("service", "phase"))
        self.retrieval_events = r.counter("llm_slo_agent_retrieval_events_total",
                                          "Retrieval SLI events: out_of_group, invalid (ttft NaN or negative), no_breakdown "
                                          "(no retrieval time), extra (a breakdown on a record whose SLI was counted "
                                          "already), exceeds_ttft (retrieval above the TTFT).", ("reason",))
        self.load_events = r.counter("llm_slo_agent_load_events_total",
                                     "Load SLI events: out_of_group (a group beyond the window's), invalid (a duration NaN, "
                                     "negative or above a day), no_time, future (starting or ending ahead of the cut), "
                                     "too_old, clipped (started before the ring), long (longer than --load-settle-ms).",
                                     ("reason",))
        # GPU signals' value distributions (the window histograms the decode kernel builds)
        self.gpu_hist = {s.slot: r.histogram(f"llm_ebpf_{s.name}", f"{s.name} values observed from GPU signal records.",
                                             s.buckets)
                         for s in catalog.SIGNALS if s.gpu and s.buckets}
        self.up.set(1)
        for k in EVENT_KINDS:
            self.kind.set(1 if k == event_kind else 0, k)
        for m in catalog.CAPABILITY_MODES:
            self.mode.set(1 if m == capability_mode else 0, m)
        for reason in DROP_REASONS:
            self.dropped.inc(0, reason)
        self.set_enabled_signals(supported, enabled)

    def set_heartbeat(self, ts_s: float = 0.0) -> None:
        self.heartbeat.set(float(int(ts_s or time.time())))

    def set_cpu_overhead(self, pct: float) -> None:
        self.cpu.set(max(0.0, pct))

    def set_rss(self) -> None:
        try:
            with open("/proc/self/statm") as f:
                self.rss.set(float(int(f.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")))
        except (OSError, ValueError, IndexError):
            pass
        from ..utils import cgroupmem

        cg = cgroupmem.reading()
        if cg is not None:
            self.cg_mem.set(float(cg["charged_bytes"]))

    def set_enabled_signals(self, supported: Iterable[str], enabled: Iterable[str]) -> None:
        en = set(enabled)
        for s in supported:
            self.sig_enabled.set(1 if s in en else 0, s)

    def observe_probe_event(self, ev: ProbeEventV1, real_probe_metrics: bool = True) -> None:
        self.probe_events.inc(1, ev.signal, ev.status)
        if real_probe_metrics and ev.signal == "dns_latency_ms":
            self.dns.observe(ev.value, _nz(ev.node, "unknown-node"), _nz(ev.pod, "unknown-pod"),
                             _nz(ev.namespace, "default"))

    def inc_dropped(self, reason: str) -> None:
        self.dropped.inc(1, reason)

    def inc_hello(self, node: str, pod: str, comm: str, count: int) -> None:
        if count:
            self.hello.inc(float(count), _nz(node, "unknown-node"), _nz(pod, "unknown-pod"), _nz(comm, "unknown"))

    # ---- GPU window outputs -------------------------------------------------------------
    def observe_window(self, hist: np.ndarray, status: np.ndarray, dbg, n_events: int, latency_ms: float,
                       node: str, pod: str, namespace: str, value_sums_milli=None) -> None:
        """hist [16 slots x 16 buckets], status [16 x 3], value sums (1/1000 unit) per slot from the
        window packet."""
        self.win_total.inc()
        self.win_events.inc(float(n_events))
        self.win_latency.observe(latency_ms)
        dns = catalog.BY_NAME["dns_latency_ms"].slot
        h = np.asarray(hist[dns], dtype=np.float64)
        nref = len(catalog.REF_DNS_BUCKETS)
        ref_counts = list(h[:nref]) + [float(h[nref:].sum())]  # buckets above 800 -> +Inf
        self.dns.add_counts(ref_counts, 0.0, _nz(node, "unknown-node"), _nz(pod, "unknown-pod"),
                            _nz(namespace, "default"))
        for slot, hm in self.gpu_hist.items():
            row = np.asarray(hist[slot], dtype=np.float64)
            nb = len(hm.buckets)
            if row[: nb + 1].sum():
                total = float(value_sums_milli[slot]) * 1e-3 if value_sums_milli is not None else 0.0
                hm.add_counts(list(row[:nb - 1]) + [float(row[nb - 1:].sum())], total)
        names = ("ok", "warning", "error")
        for s in catalog.SIGNALS:
            row = status[s.slot]
            for k in range(3):
                if row[k]:
                    self.probe_events.inc(float(row[k]), s.name, names[k])
        cand, low, overlap, dropped, enriched = (int(x) for x in list(dbg)[:5])
        d = list(dbg)
        if len(d) > 6:  # the multi-GPU exchange's losses (mislo_packet.h kDbgXchgDropped / kDbgImportDropped)
            if d[5]:
                self.dropped.inc(float(d[5]), "xchg_cap")
            if d[6]:
                self.dropped.inc(float(d[6]), "import_cap")
        self.corr.inc(float(cand), "candidate")
        self.corr.inc(float(max(0, low - overlap)), "low_confidence")
        self.corr.inc(float(dropped), "fanout_dropped")
        self.corr.inc(float(enriched), "span_enriched")

    def set_ring(self, ring_stats: dict, ring_state: dict, host_us: float) -> None:
        """Per-window ring accounting (counted on the device): id definitions applied, windows
        that met a record still being written, backlog, drops (the emulated ring counts failed
        reservations; the kernel's are invisible to user space), host time per window."""
        self.ring_defs.inc(float(ring_state.get("def_ctx", 0) + ring_state.get("def_trace", 0)))
        if ring_state.get("first_busy", -1) >= 0:
            self.ring_busy.inc()
        if ring_stats:
            self.ring_backlog.set(float(ring_stats.get("producer_pos", 0) - ring_stats.get("consumer_pos", 0)))
            self.ring_dropped.set(float(ring_stats.get("dropped", 0)))
        self.host_us.set(float(host_us))

    def set_otlp(self, receiver, mapper) -> None:
        """The OTLP receiver's and span mapper's running counts (collector/otlp.py)."""
        for outcome, v in (("accepted", getattr(receiver, "accepted", 0)), ("dropped", getattr(receiver, "dropped", 0)),
                           ("rejected", getattr(receiver, "rejected", 0)), ("conflict", getattr(mapper, "conflicts", 0)),
                           ("spoofed", getattr(mapper, "spoofed", 0)),
                           ("first_token_late", getattr(mapper, "early_dropped", 0))):
            self.otlp.set(float(v), outcome)

    def observe_open_requests(self, deadline: np.ndarray, stats: dict, names) -> None:
        """One window of the open-request tracker: ``deadline`` [G, 2] (this window's, earlier
        windows'), ``stats`` by name (pipeline/openreq.py STATS)."""
        d = np.asarray(deadline, dtype=np.int64).sum(axis=1).tolist()
        for g, n in enumerate(d):
            if n:
                self.deadline_breaches.inc(float(n), names[g] if g < len(names) else f"group-{g}")
        for state in ("open", "counted", "resolved"):
            self.open_requests.set(float(stats.get("live_" + state, 0)), state)
        for reason in ("dup_start", "start_after_sli", "dropped_full", "expired", "false_deadline"):
            self.open_events.inc(float(stats.get(reason, 0)), reason)

    def observe_ttft(self, res: dict, stats: dict, names) -> None:
        """One window of the TTFT sketch: ``res`` carries ttft_n / ttft_sum_ms / ttft_le / ttft_q /
        ttft_q_roll / ttft_n_roll per group (pipeline/slisketch.py RESULT_KEYS), ``stats`` by name."""
        from ..pipeline.slisketch import EVENT_STATS, QUANTILE_NAMES

        n, n_roll = np.asarray(res["ttft_n"]).tolist(), np.asarray(res["ttft_n_roll"]).tolist()
        for g, cnt in enumerate(n):
            svc = names[g] if g < len(names) else f"group-{g}"
            if cnt:
                self.ttft_hist.add_counts(np.asarray(res["ttft_le"][g], dtype=np.float64).tolist(),
                                          float(res["ttft_sum_ms"][g]), svc)
            for scope, have, q in (("window", cnt, res["ttft_q"][g]), ("rolling", n_roll[g], res["ttft_q_roll"][g])):
                if have:  # an empty scope keeps its last value: NaN would break rate() and max()
                    for name, v in zip(QUANTILE_NAMES, np.asarray(q, dtype=np.float64).tolist()):
                        self.ttft_quantile.set(v, svc, name, scope)
        for reason in EVENT_STATS:
            self.ttft_events.inc(float(stats.get(reason, 0)), reason)

    def observe_exemplars(self, res: dict, stats: dict, names) -> None:
        """One window of the exemplar tracker: ``res`` carries ex_k_win / ex_win per group
        (pipeline/exemplars.py RESULT_KEYS), ``stats`` by name."""
        from ..pipeline.exemplars import EVENT_STATS

        for g, have in enumerate(np.asarray(res["ex_k_win"]).tolist()):
            if have:  # a window without a record keeps the last value: NaN would break max()
                v = float(res["ex_win"][g][0]["ttft_ms"])
                self.ttft_max.set(v, names[g] if g < len(names) else f"group-{g}")
        for reason in EVENT_STATS:
            self.exemplar_events.inc(float(stats.get(reason, 0)), reason)

    def observe_pods(self, res: dict, stats: dict, names) -> None:
        """One window of the pod-breakdown tracker: ``res`` carries the pod_rec_* arrays per group
        (pipeline/podrank.py RESULT_KEYS), ``stats`` by name."""
        from ..pipeline.podrank import EVENT_STATS

        for g, seen in enumerate(np.asarray(res["pod_rec_pods"]).tolist()):
            name = names[g] if g < len(names) else f"group-{g}"
            breaches = int(res["pod_rec_b"][g])
            self.pods_seen.set(float(seen), name)
            self.pods_breaching.set(float(res["pod_rec_pods_b"][g]), name)
            worst = int(res["pod_rec_top"][g][0]["b"]) if int(res["pod_rec_k_top"][g]) else 0
            self.top_pod_share.set(worst / breaches if breaches else 0.0, name)
        for reason in EVENT_STATS:
            self.pod_events.inc(float(stats.get(reason, 0)), reason)

    def observe_onset(self, res: dict, stats: dict, names, t_ns: int, bin_ns: int) -> None:
        """One window of the breach-onset tracker: ``res`` carries ``onset_rows`` per group
        (pipeline/onset.py ONSET_ROW), ``stats`` by name; ``t_ns`` the window's cut, ``bin_ns`` a bin."""
        from ..pipeline.onset import EVENT_STATS

        rows = res["onset_rows"]
        for g in range(len(rows)):
            name = names[g] if g < len(names) else f"group-{g}"
            state = int(rows[g]["state"])
            age = max(0.0, (int(t_ns) - int(rows[g]["onset_q"]) * int(bin_ns)) * 1e-9) if state else 0.0
            self.onset_age.set(age, name)
            self.onset_state.set(float(state), name)
        for reason in EVENT_STATS:
            self.onset_events.inc(float(stats.get(reason, 0)), reason)

    def observe_decode(self, res: dict, stats: dict, names) -> None:
        """One window of the decode SLI tracker: ``res`` carries the decode_* arrays per group
        (pipeline/decodesli.py RESULT_KEYS), ``stats`` by name."""
        from ..pipeline.decodesli import CELLS, EVENT_STATS, QUANTILE_NAMES

        roll = np.asarray(res["decode_cells_roll"], dtype=np.int64)
        for g, cells in enumerate(np.asarray(res["decode_cells"], dtype=np.int64).tolist()):
            name = names[g] if g < len(names) else f"group-{g}"
            for outcome, n in zip(CELLS, cells):
                if n:
                    self.decode_requests.inc(float(n), name, outcome)
            n_roll = int(roll[g].sum())
            if n_roll:  # an empty horizon keeps its last values: NaN would break rate() and min()
                self.goodput.set(float(roll[g, 0]) / n_roll, name)
                for q, v in zip(QUANTILE_NAMES, np.asarray(res["decode_q_roll"][g], dtype=np.float64).tolist()):
                    self.tpot_quantile.set(v, name, q)
        for reason in EVENT_STATS:
            self.decode_events.inc(float(stats.get(reason, 0)), reason)

    def observe_drift(self, res: dict, stats: dict, names) -> None:
        """One window of the TTFT drift tracker: ``res`` carries the drift_* arrays per group
        (pipeline/drift.py RESULT_KEYS), ``stats`` by name."""
        from ..pipeline.drift import EVENT_STATS, FAST, SLOW, WARMING, summary

        for g, st in enumerate(np.asarray(res["drift_state"], dtype=np.int64).tolist()):
            name = names[g] if g < len(names) else f"group-{g}"
            self.drift_state.set(3.0 if st & WARMING else 1.0 if st & SLOW else 2.0 if st & FAST else 0.0, name)
            s = summary(st, res["drift_hold"][g], res["drift_n_recent"][g], res["drift_n_base"][g], res["drift_slow_num"][g],
                        res["drift_q_recent"][g], res["drift_q_base"][g])
            if s["distance"] is not None:  # an empty sample keeps the last values: NaN would break max()
                self.drift_distance.set(float(s["distance"]), name)
            if s["shift_ratio"] is not None:
                self.drift_ratio.set(float(s["shift_ratio"]), name)
        for reason in EVENT_STATS:
            self.drift_events.inc(float(stats.get(reason, 0)), reason)

    def observe_errors(self, res: dict, stats: dict, names, pairs, budget_ppm: int, bad_mask: int) -> None:
        """One window of the error SLI tracker: ``res`` carries the err_* arrays per group
        (pipeline/errsli.py RESULT_KEYS), ``stats`` by name; ``pairs`` as (long windows, short windows,
        factor_milli)."""
        from ..pipeline.errsli import CLASSES, EVENT_STATS, burn_rate

        roll = np.asarray(res["err_counts_roll"], dtype=np.int64)
        sums = np.asarray(res["err_pair_sums"], dtype=np.int64)
        firing = np.asarray(res["err_firing"], dtype=np.int64)
        bad_cols = [j for j in range(len(CLASSES)) if (bad_mask >> j) & 1]
        for g, counts in enumerate(np.asarray(res["err_counts"], dtype=np.int64).tolist()):
            name = names[g] if g < len(names) else f"group-{g}"
            for outcome, n in zip(CLASSES, counts):
                if n:
                    self.outcomes.inc(float(n), name, outcome)
            n_roll = int(roll[g].sum())
            if n_roll:  # a service without a request keeps its last value
                self.error_ratio.set(float(roll[g, bad_cols].sum()) / n_roll, name)
            for p, (L, S, f) in enumerate(pairs):
                label = f"{L}:{S}:{f / 1000.0:g}"
                for k, window in enumerate(("long", "short")):
                    b = burn_rate(int(sums[g, p, 2 * k]), int(sums[g, p, 2 * k + 1]), budget_ppm)
                    if b is not None:
                        self.error_burn.set(b, name, label, window)
                self.error_firing.set(float((int(firing[g]) >> p) & 1), name, label)
        for reason in EVENT_STATS:
            self.error_events.inc(float(stats.get(reason, 0)), reason)

    def observe_saturation(self, res: dict, stats: dict, names) -> None:
        """One window of the saturation curve tracker: ``res`` carries ``sat_rows`` / ``sat_curve`` per group
        (pipeline/satcurve.py SAT_ROW), ``stats`` by name."""
        from ..pipeline.satcurve import EVENT_STATS, summary

        for g, row in enumerate(res["sat_rows"]):
            name = names[g] if g < len(names) else f"group-{g}"
            s = summary(row, res["sat_curve"][g])
            self.saturation_state.set(float(int(row["state"])), name)
            if s["knee_concurrency"] is not None:  # a row without a knee keeps its last values
                self.saturation_knee.set(float(s["knee_concurrency"]), name)
                if s["headroom"] is not None:
                    self.saturation_headroom.set(float(s["headroom"]), name)
        for reason in EVENT_STATS:
            self.saturation_events.inc(float(stats.get(reason, 0)), reason)

    def observe_retrieval(self, res: dict, stats: dict, names) -> None:
        """One window of the retrieval SLI tracker: ``res`` carries the retr_* arrays per group
        (pipeline/retrsli.py RESULT_KEYS), ``stats`` by name."""
        from ..pipeline.retrsli import CELLS, EVENT_STATS, QUANTILE_NAMES

        roll = np.asarray(res["retr_cells_roll"], dtype=np.int64)
        for g, cells in enumerate(np.asarray(res["retr_cells"], dtype=np.int64).tolist()):
            name = names[g] if g < len(names) else f"group-{g}"
            for phase, n in zip(CELLS, cells):
                if n:
                    self.ttft_breach_phase.inc(float(n), name, phase)
            self.ttft_phase_state.set(float(int(res["retr_state"][g])), name)
            if int(roll[g].sum()):  # an empty horizon keeps its last values: NaN would break rate() and min()
                for q, v, m in zip(QUANTILE_NAMES, np.asarray(res["retr_q_roll"][g], dtype=np.float64).tolist(),
                                   np.asarray(res["retr_model_q_roll"][g], dtype=np.float64).tolist()):
                    self.retrieval_quantile.set(v, name, q)
                    self.model_ttft_quantile.set(m, name, q)
                total = float(res["retr_ttft_sum_ms_roll"][g])
                if total > 0:
                    self.retrieval_share.set(float(res["retr_sum_ms_roll"][g]) / total, name)
        for reason in EVENT_STATS:
            self.retrieval_events.inc(float(stats.get(reason, 0)), reason)

    def observe_load(self, res: dict, stats: dict, names, bin_us: int, recent_bins: int) -> None:
        """One window of the load SLI tracker: ``res`` carries ``load_rows`` per group (pipeline/loadsli.py
        LOAD_ROW), ``stats`` by name; a bin's length and the recent range's bins."""
        from ..pipeline.loadsli import EVENT_STATS, summary

        for g, row in enumerate(res["load_rows"]):
            name = names[g] if g < len(names) else f"group-{g}"
            s = summary(row, bin_us, recent_bins)
            self.load_state.set(float(int(row["state"])), name)
            self.concurrency.set(float(s["concurrency"]["peak"]), name, "peak")
            for rng in ("recent", "base"):  # a warming row keeps the last values
                if s["arrivals_per_s"][rng] is not None:
                    self.request_rate.set(float(s["arrivals_per_s"][rng]), name, rng)
                if s["concurrency"][rng] is not None:
                    self.concurrency.set(float(s["concurrency"][rng]), name, rng)
        for reason in EVENT_STATS:
            self.load_events.inc(float(stats.get(reason, 0)), reason)

    def observe_attribution(self, domain: str) -> None:
        self.attr.inc(1, domain)

    def observe_incident(self, domain: str, emitted: bool) -> None:
        self.scored.inc(1, domain, "true" if emitted else "false")
