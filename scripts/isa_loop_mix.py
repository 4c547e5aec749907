"""A per-loop instruction census of the kernels of one .hip source, from its gfx950 assembly.

Compiles the source with the project's own flags (__graft_entry__: HIPCC_FLAGS + EXTRA_FLAGS) plus -S and
-Rpass-analysis=kernel-resource-usage (hipcc cross-compiles: no GPU needed) and prints, per kernel whose mangled name contains one
of the given substrings:

  * the compiler's resource remark: VGPRs, SGPRs, SGPR / VGPR spills, scratch, LDS, occupancy;
  * one line for the whole kernel and one per loop body.  A loop is a backward branch: the instructions from the branch's target
    label to the branch.  Loops nest by containment; a loop's line counts the instructions of its OWN body ("excl": without the
    loops inside it -- what executes once per trip of this loop and no more often) and of everything inside it ("incl").

Columns: all instructions, VALU (every v_* instruction), v_mov_b32, v_readlane + v_writelane, v_readfirstlane, v_cndmask, s_nop,
s_waitcnt.  Multiply a loop's excl counts by its trip count (DESIGN.md 4 has the per-parent ones of the bench cloud) to rank the bodies.

The tool reads assembly text only.

usage: python scripts/isa_loop_mix.py hem_select.hip k_select
       python scripts/isa_loop_mix.py --csrc /path/to/another/checkout/csrc hem_select.hip k_select
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

COLS = ("all", "VALU", "v_mov", "lane", "rfl", "cndmask", "s_nop", "waitcnt")
REMARK_KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
               "Occupancy [waves/SIMD]")


def compile_asm(source: str, csrc: str):
    """-> (assembly text, the compiler's remarks)"""
    src = os.path.join(csrc, source)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        flags = [f for f in ge.HIPCC_FLAGS if f != "-fPIC"] + ge.EXTRA_FLAGS.get(source, [])
        r = subprocess.run([ge._hipcc()] + flags + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", out, src],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + r.stdout)
        with open(out) as f:
            return f.read(), r.stdout


def remarks(text: str):
    """{function name: {key: value}} from the kernel-resource-usage remarks"""
    res, cur = {}, None
    for line in text.split("\n"):
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*?): (\S+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return res


def classify(op: str):
    c = dict.fromkeys(COLS, 0)
    c["all"] = 1
    if op.startswith("v_"):
        c["VALU"] = 1
        if op.startswith("v_mov_b32"):
            c["v_mov"] = 1
        elif op.startswith(("v_readlane", "v_writelane")):
            c["lane"] = 1
        elif op.startswith("v_readfirstlane"):
            c["rfl"] = 1
        elif op.startswith("v_cndmask"):
            c["cndmask"] = 1
    elif op == "s_nop":
        c["s_nop"] = 1
    elif op == "s_waitcnt":
        c["waitcnt"] = 1
    return c


def census(body: str):
    """-> (instructions [(op, operands)], loops [(first, last, depth)] sorted by position)"""
    insts, labels = [], {}
    for raw in body.split("\n"):
        l = raw.split(";")[0].strip()
        if not l:
            continue
        m = re.match(r"^(\.?[A-Za-z_][\w.$]*):", l)
        if m:
            labels[m.group(1)] = len(insts)
            continue
        if l.startswith("."):                        # a directive
            continue
        parts = l.split(None, 1)
        insts.append((parts[0], parts[1] if len(parts) > 1 else ""))
    loops = {}
    for i, (op, args) in enumerate(insts):
        if op.startswith(("s_cbranch", "s_branch")):
            t = labels.get(args.strip())
            if t is not None and t <= i:            # a backward branch: [target, branch] is a loop body
                loops[t] = max(loops.get(t, t), i)   # several back edges to one header: the widest
    spans = sorted(loops.items())
    out = []
    for a, b in spans:
        depth = sum(1 for a2, b2 in spans if (a2, b2) != (a, b) and a2 <= a and b <= b2)
        out.append((a, b, depth))
    return insts, out


def add(into, c):
    for k in COLS:
        into[k] += c[k]


def report(name, body, rem, out):
    insts, loops = census(body)
    out.write(f"{name}\n")
    if rem:
        out.write("    " + "  ".join(f"{k}: {rem.get(k, '?')}" for k in REMARK_KEYS) + "\n")
    cls = [classify(op) for op, _ in insts]
    owner = [None] * len(insts)                      # innermost loop of every instruction
    for n, (a, b, depth) in enumerate(loops):
        for i in range(a, b + 1):
            if owner[i] is None or loops[owner[i]][2] < depth:
                owner[i] = n
    hdr = "    %-28s %-5s" % ("body", "") + "".join("%9s" % c for c in COLS)
    out.write(hdr + "\n")
    tot, outside = dict.fromkeys(COLS, 0), dict.fromkeys(COLS, 0)
    for i, c in enumerate(cls):
        add(tot, c)
        if owner[i] is None:
            add(outside, c)
    out.write("    %-28s %-5s" % ("kernel", "incl") + "".join("%9d" % tot[c] for c in COLS) + "\n")
    out.write("    %-28s %-5s" % ("  outside every loop", "excl") + "".join("%9d" % outside[c] for c in COLS) + "\n")
    for n, (a, b, depth) in enumerate(loops):
        incl, excl = dict.fromkeys(COLS, 0), dict.fromkeys(COLS, 0)
        for i in range(a, b + 1):
            add(incl, cls[i])
            if owner[i] == n:
                add(excl, cls[i])
        tag = "  " * (depth + 1) + f"loop {n} @{a}-{b}"
        out.write("    %-28s %-5s" % (tag, "excl") + "".join("%9d" % excl[c] for c in COLS) + "\n")
        if any(a <= a2 and b2 <= b and (a2, b2) != (a, b) for a2, b2, _ in loops):
            out.write("    %-28s %-5s" % ("", "incl") + "".join("%9d" % incl[c] for c in COLS) + "\n")
    out.write("\n")


def main(argv):
    csrc = ge.CSRC
    if len(argv) >= 2 and argv[0] == "--csrc":
        csrc, argv = argv[1], argv[2:]
    if not argv:
        print(__doc__)
        return 2
    s, rtext = compile_asm(argv[0], csrc)
    rem = remarks(rtext)
    want = argv[1:]
    for m in re.finditer(r"^(_Z[^\n:]+):[^\n]*\n(.*?)\.end_amdhsa_kernel", s, re.S | re.M):
        name = m.group(1)
        if want and not any(w in name for w in want):
            continue
        body = m.group(2).split(".section")[0]       # the code ends where the kernel descriptor's section begins
        report(name, body, rem.get(name, {}), sys.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
