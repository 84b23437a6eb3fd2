# dispatches per kernel name from a rocprofv3 kernel trace (tools/lockstep_trace.py): python tools/dispatch_count.py DIR n_frames
import csv, glob, sys, collections, re
d, n = sys.argv[1], int(sys.argv[2])
c = collections.Counter()
for f in glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        name = re.sub(r"\(anonymous namespace\)::", "", r["Kernel_Name"])
        m = re.search(r"(k_[A-Za-z0-9_]+|__amd_[A-Za-z0-9_]+)", name)
        c[m.group(1) if m else name[:60]] += 1
print(f"{d}: {sum(c.values())} dispatches in all = {sum(c.values()) / (n - 1):.1f} per frame index")
for k, v in sorted(c.items(), key=lambda kv: -kv[1]):
    print(f"   {v:7d}  {k}")
