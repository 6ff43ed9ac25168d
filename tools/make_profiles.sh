#!/bin/bash
# Produce the rocprofv3 evidence for bench.py (run on the GPU box from the repo root):
#   1. kernel-trace + stats of the benchmark command     -> gpurun_out/profiles/bench_kernel_stats.csv
#   2. PMC pass FETCH_SIZE, PMC pass WRITE_SIZE (separate) -> HBM bytes per launch of the Lloyd kernel
export TMPDIR=/tmp
out=$PWD/gpurun_out/profiles
rm -rf $out; mkdir -p $out
CMD="python bench.py --steps 3 --warmup 1 --full --no-cpu-baseline"
python bench.py --steps 10 --warmup 2 --full > $out/bench_plain.json 2> $out/bench_plain.err
python bench.py --config 4 --steps 10 --warmup 3 --full > $out/bench_config4.json 2> $out/bench_config4.err
python tools/time_sort.py > $out/sort_times.txt 2>&1
python tools/time_assign.py > $out/assign_times.txt 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $out/trace -- $CMD > $out/bench_under_trace.json 2>/dev/null
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $out/pmc_fetch -- $CMD > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $out/pmc_write -- $CMD > /dev/null 2>&1
python - <<'PY'
import csv, glob, json, os
out = os.path.join(os.getcwd(), "gpurun_out", "profiles")
ks = glob.glob(os.path.join(out, "trace", "**", "*kernel_stats.csv"), recursive=True)[0]
rows = list(csv.DictReader(open(ks)))
with open(os.path.join(out, "bench_kernel_stats.csv"), "w") as f:
    w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
    w.writeheader()
    for r in rows:
        w.writerow(r)
def pmc(sub, counter):
    f = glob.glob(os.path.join(out, sub, "**", "*counter_collection.csv"), recursive=True)[0]
    vals = {}
    for r in csv.DictReader(open(f)):
        if r["Counter_Name"] == counter:
            vals.setdefault(r["Kernel_Name"], []).append(float(r["Counter_Value"]))
    return vals
fetch, write = pmc("pmc_fetch", "FETCH_SIZE"), pmc("pmc_write", "WRITE_SIZE")
summ = {}
for name, v in fetch.items():
    if name.startswith("void k_") or name.startswith("k_"):
        v = sorted(v)
        # keep launches that did real work (iterations enqueued after convergence return at once)
        live = [x for x in v if x > 0.6 * v[len(v) // 2]] or v
        summ[name[:60]] = {"launches": len(live), "FETCH_SIZE_KB_mean": sum(live) / len(live)}
for name, v in write.items():
    if name[:60] in summ:
        summ[name[:60]]["WRITE_SIZE_KB_mean"] = sum(v) / len(v)
json.dump(summ, open(os.path.join(out, "pmc_hbm_summary.json"), "w"), indent=1)
def hbm(prefix):
    ks = [k for k in summ if prefix in k]
    if not ks:
        return None
    s = summ[ks[0]]
    # gfx950: FETCH_SIZE counts 64 B per 128-B request of a wide coalesced stream -> x2 (MI355X_MICROARCH.md, HBM)
    return 2.0 * s["FETCH_SIZE_KB_mean"] * 1024 + s.get("WRITE_SIZE_KB_mean", 0.0) * 1024
traffic = hbm("k_assign<1")
def raw(prefix):
    ks = [k for k in summ if prefix in k]
    return None if not ks else {"launches": summ[ks[0]]["launches"], "FETCH_SIZE_bytes": summ[ks[0]]["FETCH_SIZE_KB_mean"] * 1024, "WRITE_SIZE_bytes": summ[ks[0]].get("WRITE_SIZE_KB_mean", 0.0) * 1024}
json.dump({"k_assign_labels_hbm_bytes_per_launch": traffic,
           "sort_kernels_raw_counters": {"k_os_prep<true>": raw("k_os_prep<true"), "k_os_pass<9, 0, 0>": raw("k_os_pass<9, 0, 0"), "k_os_pass<9, 0, 1>": raw("k_os_pass<9, 0, 1"),
                                         "note": "bench vector: 25 M weights, 8 035 375 keys. Algorithmic bytes: prep 100.0 MB read + 32.1 MB keys written; a key pass 32.1 MB read + 32.1 MB written; "
                                                 "the last pass 32.1 MB read + 100.0 MB written (the values and the block of zeros). FETCH_SIZE counts 64 B per 128-B request for 16 B / lane "
                                                 "streams (the prep kernel); the passes read one dword a lane, for which the counter is not calibrated (MI355X_MICROARCH.md, HBM)"},
           "k_assign_accumulate_hbm_bytes_per_launch": hbm("k_assign<0"),
           "k_bounds_hbm_bytes_per_launch": hbm("k_bounds"),
           "k_threshold_hbm_bytes_per_launch": hbm("k_threshold"),
           "how": "rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE in separate passes over `python bench.py --steps 3 --warmup 1 --full --no-cpu-baseline`; "
                  "bytes = 2 * FETCH_SIZE_KB * 1024 (gfx950 half-count correction for 16 B/lane streaming reads) + WRITE_SIZE_KB * 1024; mean over the live launches"},
          open(os.path.join(out, "traffic.json"), "w"), indent=1)
print(json.dumps(summ, indent=1)[:1500])
print("traffic", traffic)
PY
head -12 $out/bench_kernel_stats.csv | cut -c1-200
cat $out/bench_plain.json | cut -c1-600
rm -rf $out/trace $out/pmc_fetch $out/pmc_write
