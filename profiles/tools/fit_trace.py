"""Start and end of every fit launch of each refit of a rocprofv3 --kernel-trace run, relative to the start of its k_fit_runs."""
import csv
import glob
import sys

f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
rows = [r for r in csv.DictReader(open(f)) if "k_fit_" in r["Kernel_Name"] or "k_mix_consts" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
t0 = None
for r in rows:
    n = r["Kernel_Name"].replace("tw::", "").replace("void ", "").split("(")[0]
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    if "k_fit_runs" in n:
        t0 = s
        print("-- refit")
    if t0 is None:
        continue
    print("%-20s start %8.3f end %8.3f  (%7.3f ms)  queue %s" % (n, (s - t0) / 1e6, (e - t0) / 1e6, (e - s) / 1e6, r.get("Queue_Id", "?")))
