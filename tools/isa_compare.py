#!/usr/bin/env python3
"""Compare two gfx950 assembly files (hipcc ... --cuda-device-only -S) kernel by kernel.

    tools/isa_compare.py OLD.s NEW.s [--rename REGEX REPLACEMENT]... [--all]

Per kernel symbol: the instruction count of both, whether the instruction text is identical, whether the multiset of
opcodes is equal, and the five resource fields of the kernel descriptor (next_free_vgpr, next_free_sgpr,
accum_offset, group_segment_fixed_size, private_segment_fixed_size).  --rename rewrites the demangled names of OLD
before the kernels are paired (a kernel that was renamed or merged); it may be given several times.  Rows are printed
for the kernels that differ in anything (--all: for every kernel), then the totals.  Exit status 1 if the kernel sets
differ or any kernel differs in count, opcodes or resources.
"""
import argparse
import collections
import re
import shutil
import subprocess
import sys

FIELDS = ["next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size"]


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if tool is None:
        raise SystemExit("isa_compare: needs llvm-cxxfilt or c++filt on PATH")
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def parse(path):
    """{mangled kernel symbol: (instructions [str], {field: value})}"""
    body, res = {}, {}
    cur = desc = None
    with open(path) as f:
        for raw in f:
            line = raw.split(";", 1)[0].strip()
            if not line:
                continue
            if line.startswith(".amdhsa_kernel "):
                desc = line.split()[1]
                res[desc] = {}
            elif line == ".end_amdhsa_kernel":
                desc = None
            elif desc is not None:
                m = re.match(r"\.amdhsa_(\w+)\s+(\S+)", line)
                if m and m.group(1) in FIELDS:
                    res[desc][m.group(1)] = m.group(2)
            elif re.match(r"^[A-Za-z_][\w$.]*:$", line) and not line.startswith(".L"):
                cur = line[:-1]
                body[cur] = []
            elif line.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None and not line.startswith(".") and not line.endswith(":"):
                body[cur].append(" ".join(line.split()))
    return {k: (body.get(k, []), res[k]) for k in res}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPL"))
    ap.add_argument("--all", action="store_true")
    a = ap.parse_args()
    old, new = parse(a.old), parse(a.new)
    names = demangle(sorted(set(old) | set(new)))

    def key(sym, renames):
        n = names[sym]
        for rx, rp in renames:
            n = re.sub(rx, rp, n)
        return n

    ko = collections.defaultdict(list)
    for s in old:
        ko[key(s, a.rename)].append(s)
    kn = {key(s, []): s for s in new}
    clash = {k: v for k, v in ko.items() if len(v) > 1}
    only_old = sorted(set(ko) - set(kn))
    only_new = sorted(set(kn) - set(ko))
    print(f"kernels: old {len(old)}, new {len(new)}, paired {len(set(ko) & set(kn))}, renamed "
          f"{sum(1 for k, v in ko.items() if names[v[0]] != k)}")
    for k, v in clash.items():
        print(f"CLASH  {len(v)} old kernels map to {k}")
    for k in only_old:
        print(f"ONLY OLD  {k}")
    for k in only_new:
        print(f"ONLY NEW  {k}")
    n_text = n_ops = n_cnt = n_res = 0
    print("# count_old count_new text opcodes resources(" + ",".join(FIELDS) + ") kernel")
    for k in sorted(set(ko) & set(kn)):
        (bo, ro), (bn, rn) = old[ko[k][0]], new[kn[k]]
        text = bo == bn
        ops = collections.Counter(i.split()[0] for i in bo) == collections.Counter(i.split()[0] for i in bn)
        cnt = len(bo) == len(bn)
        res = ro == rn
        n_text += text
        n_ops += ops
        n_cnt += cnt
        n_res += res
        if a.all or not (text and ops and cnt and res):
            rs = ",".join(rn.get(f, "-") if ro.get(f) == rn.get(f) else f"{ro.get(f, '-')}->{rn.get(f, '-')}" for f in FIELDS)
            print(f"{len(bo):6d} {len(bn):6d} {'same' if text else 'DIFF'} {'equal' if ops else 'DIFF '} {rs}  {k}")
    n = len(set(ko) & set(kn))
    scratch = sum(1 for _, r in new.values() if r.get("private_segment_fixed_size", "0") != "0")
    print(f"totals over {n} paired kernels: text identical {n_text}, opcode multiset equal {n_ops}, "
          f"instruction count equal {n_cnt}, resources equal {n_res}; new kernels with scratch {scratch}")
    ok = not clash and not only_old and not only_new and n_ops == n and n_cnt == n and n_res == n
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
