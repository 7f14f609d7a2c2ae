#!/usr/bin/env python3
"""Per-iteration kernel timeline of the GEM bench from a rocprofv3
--kernel-trace CSV (run_kernel_trace.csv): for every kernel of one iteration,
its queue and the medians of start / end / duration over the last N
iterations, in us from the E-step's start.

Usage: tools/kernel_timeline.py run_kernel_trace.csv [N=40] [anchor=k_estep]"""
import csv
import re
import statistics
import sys


def short(name):
    name = re.sub(r"^void\s+", "", name)
    head = re.split(r"[<(]", name, 1)[0]
    return head.split("::")[-1].strip()


def col(row, *names):
    for n in names:
        for k in row:
            if k.lower() == n:
                return row[k]
    raise KeyError(names)


def main():
    path = sys.argv[1]
    last = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    anchor = sys.argv[3] if len(sys.argv) > 3 else "k_estep"
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            rows.append((int(col(r, "start_timestamp")), int(col(r, "end_timestamp")),
                         short(col(r, "kernel_name")), col(r, "queue_id")))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if r[2].startswith(anchor)]
    if len(starts) < last + 2:
        sys.exit("only %d anchor dispatches in the trace" % len(starts))
    starts = starts[-(last + 1):]
    queues = {}
    acc = {}
    order = []
    period = []
    for a, b in zip(starts[:-1], starts[1:]):
        t0 = rows[a][0]
        period.append((rows[b][0] - t0) / 1e3)
        seen = {}
        for s, e, name, q in rows[a:b]:
            qn = queues.setdefault(q, "q%d" % (len(queues) + 1))
            n = seen.get((name, qn), 0)
            seen[(name, qn)] = n + 1
            key = (name, qn, n)
            if key not in acc:
                acc[key] = []
                order.append(key)
            acc[key].append(((s - t0) / 1e3, (e - t0) / 1e3))
    order.sort(key=lambda k: statistics.median(x[0] for x in acc[k]))
    for key in order:
        v = acc[key]
        s = statistics.median(x[0] for x in v)
        e = statistics.median(x[1] for x in v)
        d = statistics.median(x[1] - x[0] for x in v)
        print("%-22s %s start %8.1f end %8.1f dur %7.1f  (n=%d)" % (key[0], key[1], s, e, d, len(v)))
    print("%-22s    start %8.1f  (the iteration's period)" % ("next " + anchor, statistics.median(period)))


if __name__ == "__main__":
    main()
