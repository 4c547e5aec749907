"""Kernel resource table from two sets of hipcc remarks: ``hipcc <the build's flags> -Rpass-analysis=kernel-resource-usage -c X.hip``
with stderr saved as ``<dir>/X.remarks``, once for the parent commit and once for the head.  Kernels are matched by name across
files (a kernel may have moved from one translation unit to another).

    python scripts/kernel_resource_table.py PARENT_DIR HEAD_DIR [name-substring ...] > profiles/<table>.txt
"""
import glob
import os
import re
import subprocess
import sys

FIELDS = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("SGPRs Spill", "sgpr_spill"), ("VGPRs Spill", "vgpr_spill"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "LDS"), ("Occupancy [waves/SIMD]", "occ")]


def parse(d):
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.remarks"))):
        cur = None
        for line in open(path):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {"file": os.path.basename(path)[:-8] + ".hip"})
                continue
            for label, key in FIELDS:
                m = re.search(re.escape(label) + r": (\d+)", line)
                if m and cur is not None:
                    cur[key] = int(m.group(1))
    return out


def main():
    parent, head = parse(sys.argv[1]), parse(sys.argv[2])
    want = sys.argv[3:]
    names = [n for n in sorted(set(parent) | set(head)) if not want or any(w in n for w in want)]
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n") if names else []
    keys = [k for _, k in FIELDS]
    print("%-74s %-22s %s" % ("kernel", "file parent -> head", "  ".join("%10s" % k for k in keys)))
    for n, d in zip(names, dem):
        p, h = parent.get(n), head.get(n)
        # without the anonymous namespace and the parameter list (the last parenthesis group: a template argument may hold a cast)
        short = re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", d.replace("(anonymous namespace)::", "")).replace("void ", "").replace("gsr::", "")
        cols = []
        for k in keys:
            a, b = (p or {}).get(k, "-"), (h or {}).get(k, "-")
            cols.append("%10s" % (str(a) if a == b else "%s>%s" % (a, b)))
        same = p is not None and h is not None and all(p.get(k) == h.get(k) for k in keys)
        print("%-74s %-22s %s  %s" % (short[:74], "%s -> %s" % ((p or {}).get("file", "-"), (h or {}).get("file", "-")), "  ".join(cols), "equal" if same else "CHANGED"))


if __name__ == "__main__":
    main()
