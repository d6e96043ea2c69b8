"""Per-window kernel time breakdown from a rocprofv3 ``--kernel-trace --output-format csv`` run.

One ``k_pack`` (multi-GPU) or ``k_window_end`` (one GPU) dispatch ends every window
(ops/csrc/engine.hip). With overlapped windows (the front stage of window k + 1 beside the back
stage of window k, on two streams) the dispatches between two such markers belong to two
windows, so nothing here is attributed to a window by position: over the span of the last
``--windows`` markers the table reports, per kernel and launch shape (grid / workgroup), the
summed duration and the dispatch count divided by the number of windows -- the unprofiled (no
PMC) device time each phase costs per window -- and below it the steady-state period (the
median distance between consecutive markers), how busy the kernels keep the device (the union of
their intervals over the span) and how many windows' first kernel (``k_window_begin``) started
before the previous window's marker, i.e. how often two windows really ran side by side.

    python tools/kernel_phases.py gpurun_out/prof --windows 20 --title ...
"""

import argparse
import collections
import csv
import glob
import os
import statistics

MARKERS = ("k_pack", "k_window_end")


def load(d):
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            for r in csv.DictReader(fh):
                name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
                shape = f"{r.get('Grid_Size', r.get('Grid_Size_X', '?'))}/{r.get('Workgroup_Size', r.get('Workgroup_Size_X', '?'))}"
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, shape))
    rows.sort()
    return rows


def is_marker(name, markers=MARKERS):
    return any(m in name for m in markers)


def union_us(rows):
    """Time covered by at least one of the intervals (us)."""
    busy, end = 0, None
    for s, e, *_ in sorted(rows):
        if end is None or s > end:
            busy += e - s
            end = e
        elif e > end:
            busy += e - end
            end = e
    return busy / 1e3


def summarise(d, n_last, title, prefix="mislo::"):
    rows = [r for r in load(d) if r[2].startswith(prefix)]
    marks = [r for r in rows if is_marker(r[2])]
    if len(marks) < 2:
        return f"# {title}\n\nfewer than two windows in the trace"
    # every window has one k_window_begin and one marker, each in window order on its stream: the
    # i-th of each belong to window i
    begins = [r for r in rows if "k_window_begin" in r[2]]
    paired = len(begins) == len(marks)
    # the last n + 1 windows' markers and, where they pair up, the same windows' heads
    marks = marks[-(n_last + 1):]
    begins = begins[-len(marks):] if paired else []
    n = len(marks) - 1
    ahead = sum(1 for b, prev in zip(begins[1:], marks) if b[0] < prev[0])
    t0, t1 = marks[0][1], marks[-1][1]  # from the end of one marker to the end of the last
    mine = [r for r in rows if r[0] >= t0 and r[1] <= t1]
    per = collections.defaultdict(lambda: [0.0, 0])
    for s, e, name, shape in mine:
        per[(name, shape)][0] += (e - s) / 1e3
        per[(name, shape)][1] += 1
    table = sorted(((k[0], k[1], v[1] / n, v[0] / n) for k, v in per.items()), key=lambda r: -r[3])
    total = sum(r[3] for r in table)
    period = [(b[1] - a[1]) / 1e3 for a, b in zip(marks, marks[1:])]
    out = [f"# {title}", "", f"{n} windows (the span of the last {n + 1} k_pack / k_window_end dispatches); per window.", "",
           "| kernel | grid/wg | dispatches / window | us / window | share % |", "|---|---|---|---|---|"]
    for r in table:
        out.append(f"| `{r[0]}` | {r[1]} | {r[2]:.1f} | {r[3]:.1f} | {100 * r[3] / total:.1f} |")
    out += ["", f"Sum of kernel time per window: **{total:.1f} us**; steady-state period (marker to marker): median "
                f"{statistics.median(period):.1f} us (min {min(period):.1f}, max {max(period):.1f}); the device runs at "
                f"least one of these kernels {100 * union_us(mine) / ((t1 - t0) / 1e3):.0f} % of the span; "
                + (f"{ahead} of {n} windows began (`k_window_begin`) before the previous window's marker."
                   if paired else "window heads and markers do not pair up in this trace.")]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dir")
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--title", default="per-window kernel time")
    ap.add_argument("--prefix", default="mislo::")
    a = ap.parse_args()
    print(summarise(a.dir, a.windows, a.title, a.prefix))


if __name__ == "__main__":
    main()
