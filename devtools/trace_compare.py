"""Do two libraries enqueue the same step? Compares the steady-state steps of two rocprofv3 kernel_trace.csv files (devtools/step_probe.py
under rocprofv3 --kernel-trace, once per library): per hardware queue, numbered in order of first appearance, the list of (kernel name with
template arguments, grid x/y/z, workgroup size, LDS bytes) in start order. A step begins at its k_minmax_u16 launch; a queue without one
(the side stream of a lone two-stream context) is cut at the other queue's.
  python devtools/trace_compare.py <label> <a.csv> <b.csv>     ->  one line: launches per step and "identical" or the first difference"""
import csv
import sys

KEEP = 3   # steady state: the last steps of every queue


def col(r, *names):
    for n in names:
        if r.get(n) not in (None, ""):
            return r[n]
    return "?"


def steps_of(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    queues, cuts = {}, []
    for r in rows:
        name = r["Kernel_Name"].replace("void musica::", "").replace("musica::", "")
        rec = (name, col(r, "Grid_Size_X", "Grid_Size"), col(r, "Grid_Size_Y"), col(r, "Grid_Size_Z"),
               col(r, "Workgroup_Size_X", "Workgroup_Size"), col(r, "Workgroup_Size_Y"), col(r, "Workgroup_Size_Z"), col(r, "LDS_Block_Size", "LDS_Block_Size_v"))
        if not name.startswith("k_"):
            continue   # the runtime's own fill / copy kernels (allocation, upload)
        first = name.startswith("k_minmax_u16")
        if first:
            cuts.append(int(r["Start_Timestamp"]))
        queues.setdefault(col(r, "Queue_Id"), []).append((int(r["Start_Timestamp"]), first, rec))
    out = []
    for q in sorted(queues, key=lambda q: queues[q][0][0]):
        own = any(first for _, first, _ in queues[q])
        steps = []
        nxt = 0
        for t, first, rec in queues[q]:
            cut = first
            while not own and nxt < len(cuts) and cuts[nxt] <= t:
                nxt += 1
                cut = True
            if cut:
                steps.append([])
            if steps:
                steps[-1].append(rec)
        if steps:
            out.append(steps[-KEEP:])
    return out


def main():
    label, a, b = sys.argv[1], steps_of(sys.argv[2]), steps_of(sys.argv[3])
    per_step = sum(len(q[-1]) for q in a if q)
    if len(a) != len(b):
        print("%s: %d launches per step, DIFFERENT: %d queues against %d" % (label, per_step, len(a), len(b)))
        return 1
    for qi, (qa, qb) in enumerate(zip(a, b)):
        if len(qa) != len(qb) or len(qa) < KEEP:
            print("%s: %d launches per step, DIFFERENT: queue %d has %d / %d steady steps (need %d)" % (label, per_step, qi, len(qa), len(qb), KEEP))
            return 1
        for si, (sa, sb) in enumerate(zip(qa, qb)):
            for k in range(max(len(sa), len(sb))):
                ra = sa[k] if k < len(sa) else None
                rb = sb[k] if k < len(sb) else None
                if ra != rb:
                    print("%s: %d launches per step, DIFFERENT: queue %d step -%d launch %d: %s against %s" % (label, per_step, qi, KEEP - si, k, ra, rb))
                    return 1
    print("%s: %d launches per step on %d queue(s), identical (%d steady steps per queue)" % (label, per_step, len(a), KEEP))
    return 0


if __name__ == "__main__":
    sys.exit(main())
