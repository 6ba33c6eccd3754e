"""From a rocprofv3 --kernel-trace CSV of an inference run of bench.py: the forwards of every stream (mel_kernel ... the fc GEMM), which
hardware queue each stream was given, and how many forwards execute ALONE -- while no kernel of another stream runs -- against how many
overlap with other streams' kernels, with their durations.  Streams that share a hardware queue run one after the other, so a run whose
host enqueues far ahead ends in a chain of lone forwards on the shared queue ("Two workgroup sets when alone").
Usage: python tools/trace_lone_forwards.py <dir with *_kernel_trace.csv> [forwards to skip at the start of every stream = 0]"""
import csv, glob, os, re, sys
from collections import defaultdict

root = sys.argv[1]
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 0
rows = []
for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "").replace("mt::", ""),
                     r["Queue_Id"], r["Stream_Id"]))
rows.sort()
model = [r for r in rows if re.match(r"(mel_kernel|conv1|gemm|lstm_)", r[2])]
by_stream = defaultdict(list)
for r in model:
    by_stream[r[4]].append(r)
fwd = []                                       # (start, end, stream, queue, time in recurrence launches, recurrence kernel names)
for st, ks in by_stream.items():
    first = "mel_kernel" if any(k[2].startswith("mel_kernel") for k in ks) else "conv1"
    cur = []
    mine = []
    for k in ks + [None]:
        if k is None or k[2].startswith(first):
            if cur and any(c[2].startswith("lstm_") for c in cur):
                rec = [c for c in cur if c[2].startswith("lstm_")]
                mine.append((cur[0][0], cur[-1][1], st, cur[0][3], sum(c[1] - c[0] for c in rec), sorted({c[2] for c in rec})))
            cur = []
        if k is not None:
            cur.append(k)
    fwd += mine[skip:]
if not fwd:
    sys.exit("no forward (mel_kernel / conv1 ... lstm_* ... gemm) in this trace")
fwd.sort()
t0, t1 = fwd[0][0], max(f[1] for f in fwd)
print(f"{len(fwd)} forwards on {len(by_stream)} streams, {(t1 - t0) * 1e-6:.1f} ms from the first forward's start to the last one's end")
for st in sorted(by_stream):
    mine = [f for f in fwd if f[2] == st]
    if mine:
        print(f"  stream {st}: hardware queue {mine[0][3]}, {len(mine)} forwards, last one ends at {(mine[-1][1] - t0) * 1e-6:.1f} ms")


def overlap_with_others(f):
    """ns of [start, end) of forward f during which a model kernel of another stream runs"""
    iv = sorted((max(s, f[0]), min(e, f[1])) for s, e, n, q, st in model if st != f[2] and e > f[0] and s < f[1])
    tot, hi = 0, f[0]
    for s, e in iv:
        s = max(s, hi)
        if e > s:
            tot += e - s
            hi = e
    return tot


lone, shared = [], []
for f in fwd:
    (lone if overlap_with_others(f) <= 0.01 * (f[1] - f[0]) else shared).append(f)


def line(name, fs):
    if not fs:
        print(f"{name}: none")
        return
    d = sorted((f[1] - f[0]) * 1e-6 for f in fs)
    r = sorted(f[4] * 1e-6 for f in fs)
    print(f"{name}: {len(fs)} forwards, {sum(d):.1f} ms in all; per forward min {d[0]:.2f} / median {d[len(d) // 2]:.2f} / max {d[-1]:.2f} ms, "
          f"of which recurrence launches median {r[len(r) // 2]:.2f} ms")
    print("    recurrence kernels: " + ", ".join(sorted({n for f in fs for n in f[5]})))


line("ALONE (no kernel of another stream runs during the forward, 1 % tolerance)", lone)
line("OVERLAPPED with other streams' kernels", shared)
if lone:
    print(f"the lone forwards lie between {(min(f[0] for f in lone) - t0) * 1e-6:.1f} and {(max(f[1] for f in lone) - t0) * 1e-6:.1f} ms of the {(t1 - t0) * 1e-6:.1f}-ms span: "
          f"{100.0 * sum(f[1] - f[0] for f in lone) / (t1 - t0):.0f} % of it")
