"""LM-head backward kernels of a rocprofv3 kernel trace of bench.py (C2): the kernels between each xent_kernel
and the first ln_bwd kernel after it, per stream, averaged over the traced steps after the warm-up.
usage: python tools/lmhead_kernels.py <rocprof dir> [skip-steps]"""
import csv
import sys
from collections import defaultdict

d = sys.argv[1]
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 3
rows = list(csv.DictReader(open(f"{d}/run_kernel_trace.csv")))
rows.sort(key=lambda r: int(r['Start_Timestamp']))
short = lambda n: n.split('(')[0].replace('void ', '').replace('ergm::', '')[:90]  # noqa: E731
xs = [i for i, r in enumerate(rows) if 'xent_kernel' in r['Kernel_Name']]
acc = defaultdict(list)
for i in xs[skip:]:
    t_x = int(rows[i]['Start_Timestamp'])
    j, seen = i, 0
    while j < len(rows) and seen < 14:
        r = rows[j]
        n = r['Kernel_Name']
        dur = (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
        grid = r.get('Grid_Size_X', r.get('Grid_Size', '?'))
        wg = r.get('Workgroup_Size_X', r.get('Workgroup_Size', '?'))
        acc[(seen, short(n), grid, wg, r['Stream_Id'])].append((dur, (int(r['Start_Timestamp']) - t_x) / 1e3))
        seen += 1
        j += 1
print(f"{len(xs) - skip} steps; the 14 kernels from xent_kernel on, in start order (position, name, grid, wg, stream)")
for k, v in sorted(acc.items()):
    if len(v) < (len(xs) - skip) // 2:
        continue
    print(f"#{k[0]:2d} n={len(v):2d} dur {sum(x[0] for x in v) / len(v):8.1f} us  start +{sum(x[1] for x in v) / len(v):7.1f} us "
          f" grid {k[2]:>8s} wg {k[3]:>4s} stream {k[4]:>3s}  {k[1]}")
