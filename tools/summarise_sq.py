"""Per-kernel SQ counters of a `rocprofv3 --pmc SQ_...` run (a run of its own, no tracing combined):
mean per dispatch and per wave (Grid_Size / 64), as JSON.  Usage:
  python tools/summarise_sq.py DIR/run_counter_collection.csv KERNEL_SUBSTRING [KERNEL_SUBSTRING ...]"""
import collections
import csv
import json
import re
import sys

path, subs = sys.argv[1], sys.argv[2:]
acc = {s: collections.defaultdict(float) for s in subs}
disp = {s: set() for s in subs}
waves = {s: 0 for s in subs}
names = {}
for r in csv.DictReader(open(path)):
    for s in subs:
        if s in r["Kernel_Name"]:
            names[s] = re.sub(r"\((?!anonymous namespace\)).*", "", r["Kernel_Name"])  # without the parameter list
            acc[s][r["Counter_Name"]] += float(r["Counter_Value"])
            if r["Dispatch_Id"] not in disp[s]:
                disp[s].add(r["Dispatch_Id"])
                waves[s] += int(r["Grid_Size"]) // 64
            break
out = {}
for s in subs:
    n = len(disp[s])
    if not n:
        continue
    out[s] = {"kernel": names[s], "dispatches": n, "waves_per_dispatch": waves[s] // n,
              "per_dispatch": {k: round(v / n, 1) for k, v in sorted(acc[s].items())},
              "per_wave": {k: round(v / waves[s], 2) for k, v in sorted(acc[s].items())}}
print(json.dumps(out, indent=1))
