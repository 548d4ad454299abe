#!/usr/bin/env python3
"""How many align launches ran side by side, from a rocprofv3 kernel trace (--kernel-trace, CSV output).

Reads <prefix>_kernel_trace.csv and prints, for the launches whose kernel name contains --kernel (default cvo_align_kernel):
the number of launches, the distinct hardware queue ids they ran on, the mean launch duration, and the launches side by side
= sum of the durations / span from the first start to the last end.  --skip N leaves out the first N launches (set-up and warm-up
run with gaps the timed loop does not have); --last N keeps the last N only.

usage: launch_overlap.py TRACE.csv [--kernel NAME] [--skip N] [--last N]"""
import argparse
import csv


def column(fields, *names):
    low = {f.lower(): f for f in fields}
    for n in names:
        if n.lower() in low:
            return low[n.lower()]
    raise SystemExit(f"no column of {names} in {fields}")


def summarize(path, kernel="cvo_align_kernel", skip=0, last=0):
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        name_c = column(rd.fieldnames, "Kernel_Name", "KernelName", "Name")
        q_c = column(rd.fieldnames, "Queue_Id", "QueueId", "Queue_ID")
        t0_c = column(rd.fieldnames, "Start_Timestamp", "BeginNs", "Start")
        t1_c = column(rd.fieldnames, "End_Timestamp", "EndNs", "End")
        rows = [(int(r[t0_c]), int(r[t1_c]), r[q_c]) for r in rd if kernel in r[name_c]]
    rows.sort()
    rows = rows[skip:]
    if last > 0:
        rows = rows[-last:]
    if not rows:
        raise SystemExit(f"no launches of {kernel} in {path}")
    total = sum(t1 - t0 for t0, t1, _ in rows)
    span = max(t1 for _, t1, _ in rows) - min(t0 for t0, _, _ in rows)
    queues = sorted({q for _, _, q in rows}, key=lambda q: (len(q), q))
    per_queue = {q: sum(1 for r in rows if r[2] == q) for q in queues}
    return {"launches": len(rows), "queue_ids": queues, "distinct_queues": len(queues), "launches_per_queue": per_queue,
            "mean_launch_ms": total / len(rows) / 1e6, "span_ms": span / 1e6, "side_by_side": total / span if span else float("nan")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--kernel", default="cvo_align_kernel")
    ap.add_argument("--skip", type=int, default=0)
    ap.add_argument("--last", type=int, default=0)
    a = ap.parse_args()
    s = summarize(a.trace, a.kernel, a.skip, a.last)
    print(f"{a.trace}: {s['launches']} launches of {a.kernel} on {s['distinct_queues']} hardware queues (ids {', '.join(s['queue_ids'])}; "
          f"launches per queue {s['launches_per_queue']}); mean launch {s['mean_launch_ms']:.3f} ms; span {s['span_ms']:.2f} ms; "
          f"side by side {s['side_by_side']:.2f}")


if __name__ == "__main__":
    main()
