#!/usr/bin/env python3
"""Do two `gpu_busy.py --timeline` listings queue the same work on the same streams?  Per stream, the sequence of
(kernel name, workgroups) in start order -- a stream runs its dispatches in order -- and the number of distinct streams;
timestamps are ignored.  The launch census (launch_census.py) does not see which stream a launch went to, and a lost
overlap gives correct results: this is the check of a change to the host driver's stream assignment.

  timeline_streams.py A.txt B.txt      prints the streams of A with their dispatch counts and "identical", or the first
                                       difference; exit status 0 / 1
"""
import sys


def streams(path):
    out, table = {}, False
    for line in open(path):
        f = line.split(None, 6)
        if f[:2] == ["start", "us"]:
            table = True
            continue
        if not table or len(f) < 7 or not f[0].replace(".", "").isdigit():
            continue
        out.setdefault(f[3], []).append((f[6].strip(), int(f[4])))
    return out


a, b = streams(sys.argv[1]), streams(sys.argv[2])
for st in sorted(a):
    print("stream %s: %d dispatches" % (st, len(a[st])))
if len(a) != len(b):
    sys.exit("distinct streams: %d against %d" % (len(a), len(b)))
for st in sorted(a):
    if st not in b:
        sys.exit("stream %s: only in %s" % (st, sys.argv[1]))
    for k, (x, y) in enumerate(zip(a[st], b[st])):
        if x != y:
            sys.exit("stream %s, dispatch %d: %s against %s" % (st, k + 1, x, y))
    if len(a[st]) != len(b[st]):
        sys.exit("stream %s: %d dispatches against %d" % (st, len(a[st]), len(b[st])))
print("identical: %d streams, the same (kernel, workgroups) sequence on each" % len(a))
