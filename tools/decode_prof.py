"""Kernel time of a generation run by kernel AND launch geometry, from a rocprofv3 --kernel-trace run of
tools/gen_bench.py: python tools/decode_prof.py <dir> [top].

rocprofv3's own --stats groups by kernel name only; the decode GEMMs of one step differ in shape under one name, and
the grid tells them apart (gemm configuration 0: N/64 x M/64 workgroups of 256 threads; ergm_linear_rows: N/16 x
M/32 of 512).  Prints, per (kernel, grid, workgroup): launches, total ms, mean and median us, and the sum over all
kernels, which set against the wall time of the call (gen_bench's ms_median x the runs the trace covers) is the share
of the call the GPU was busy."""
import csv
import glob
import statistics
import sys
from collections import defaultdict


def main():
    d = sys.argv[1]
    top = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    files = glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {d}")
    groups = defaultdict(list)
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"].split("(")[0][-70:]
            grid = tuple(int(r[f"Grid_Size_{a}"]) // max(1, int(r[f"Workgroup_Size_{a}"])) for a in "XYZ")
            groups[(name, grid, int(r["Workgroup_Size_X"]))].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    total = sum(sum(v) for v in groups.values())
    print(f"kernels: {sum(len(v) for v in groups.values())} launches, {total / 1e6:.2f} ms in total")
    for (name, grid, wg), v in sorted(groups.items(), key=lambda kv: -sum(kv[1]))[:top]:
        print(f"{sum(v) / 1e6:9.2f} ms {100 * sum(v) / total:5.1f} %  n {len(v):6d}  mean {statistics.mean(v) / 1e3:7.2f} us  "
              f"median {statistics.median(v) / 1e3:7.2f} us  grid {'x'.join(map(str, grid)):>12} wg {wg:4d}  {name}")


if __name__ == "__main__":
    main()
