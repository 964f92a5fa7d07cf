#!/usr/bin/env python
"""VGPR liveness of one kernel of a gfx950 assembly file (hipcc -S / -save-temps): where the register pressure peaks and what is live there.

    hipcc --offload-arch=gfx950 <the Makefile's flags> --cuda-device-only -S pt_shade_rgb_primary.hip -o shade.s
    python tools/isa_vgpr_liveness.py shade.s [KERNEL_INDEX] [LINE]

Backward data flow over the PHYSICAL registers along the control-flow graph of the labels and branches.  A write under a partial EXEC mask
counts as a full definition, as in the compiler's own liveness.  Prints the maximum, a profile of the live count per 100 instructions
(barriers marked), and — with LINE, default the line of the maximum — every register live there with the lines of its reaching definitions
and of its next uses: a value whose next use lies far behind the code in progress occupies its register for somebody else.
The count is of live registers; the allocation is higher by what register tuples and their alignment cost."""
import re
import sys

REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")
NO_DST = ("global_store", "ds_write", "ds_store", "buffer_store", "scratch_store", "flat_store", "v_cmpx", "s_", "v_nop", "buffer_wbl2", "buffer_inv")
DST_IS_USED = ("v_fmac", "v_mac", "v_writelane", "v_movrel", "v_dot", "v_pk_fmac")
WITH_DST = ("v_", "global_load", "ds_", "buffer_load", "scratch_load", "flat_load", "global_atomic", "buffer_atomic", "flat_atomic")


def regs(text):
    r = set()
    for m in REG.finditer(text):
        if m.group(1):
            r.add(int(m.group(1)))
        else:
            r.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return r


def parse(lines, start, end):
    ins, label_at = [], {}           # ins: (line number, mnemonic, defs, uses, text)
    for i in range(start + 1, end):
        m = re.match(r"^(\.LBB\d+_\d+):", lines[i])
        if m:
            label_at[m.group(1)] = len(ins)
            continue
        l = lines[i].split(";")[0].rstrip()
        if not l.startswith("\t") or l.strip().startswith("."):
            continue
        t = l.strip()
        mn = t.split()[0]
        ops = t[len(mn):].split(",")
        atomic = "atomic" in mn
        no_dst = mn.startswith(NO_DST) or (atomic and not mn.startswith("ds_") and not re.search(r"\b(glc|sc0)\b", t)) or \
            (atomic and mn.startswith("ds_") and "_rtn" not in mn)
        defs, uses = set(), set()
        for k, o in enumerate(ops):
            r = regs(o)
            if k == 0 and not no_dst and mn.startswith(WITH_DST):
                defs |= r
                if mn.startswith(DST_IS_USED) or "dpp" in t or mn.startswith("v_swap"):
                    uses |= r
            else:
                uses |= r
        if mn.startswith("v_swap"):
            defs |= regs(ops[1])
        ins.append((i + 1, mn, defs, uses, t))
    n = len(ins)
    succ = [[] for _ in range(n)]
    for k, (_, mn, _, _, t) in enumerate(ins):
        if mn == "s_endpgm":
            continue
        if mn == "s_branch":
            succ[k].append(label_at[t.split()[1]])
            continue
        if mn.startswith("s_cbranch"):
            succ[k].append(label_at[t.split()[1]])
        if k + 1 < n:
            succ[k].append(k + 1)
    return ins, succ


def main():
    lines = open(sys.argv[1]).read().split("\n")
    index = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w+:\s*(;.*)?$", l)]
    ends = [i for i, l in enumerate(lines) if ".end_amdhsa_kernel" in l]
    start = starts[index]
    end = [x for x in ends if x > start][0]
    ins, succ = parse(lines, start, end)
    n = len(ins)
    live = [set() for _ in range(n)]
    changed = True
    while changed:
        changed = False
        for k in range(n - 1, -1, -1):
            out = set()
            for x in succ[k]:
                if x < n:
                    out |= live[x]
            new = (out - ins[k][2]) | ins[k][3]
            if new != live[k]:
                live[k], changed = new, True
    peak = max(range(n), key=lambda k: len(live[k]))
    print("%s: lines %d .. %d, %d instructions" % (lines[start].rstrip(":"), start + 1, end + 1, n))
    print("most VGPRs live: %d, before line %d: %s" % (len(live[peak]), ins[peak][0], ins[peak][4]))
    for b in range(0, n, 100):
        seg = range(b, min(n, b + 100))
        print("lines %6d .. %6d  live %3d .. %3d%s" % (ins[b][0], ins[seg[-1]][0], min(len(live[j]) for j in seg), max(len(live[j]) for j in seg),
                                                      "  barrier" if any(ins[j][1] == "s_barrier" for j in seg) else ""))
    pred = [[] for _ in range(n)]
    for k in range(n):
        for x in succ[k]:
            if x < n:
                pred[x].append(k)

    def search(k, r, forward):
        seen, stack, out = set(), ([k] if forward else list(pred[k])), set()
        while stack:
            j = stack.pop()
            if j in seen:
                continue
            seen.add(j)
            if r in ins[j][3 if forward else 2]:
                out.add(ins[j][0])
                continue
            if forward and r in ins[j][2]:
                continue
            stack.extend((x for x in succ[j] if x < n) if forward else pred[j])
        return sorted(out)

    at = int(sys.argv[3]) if len(sys.argv) > 3 else ins[peak][0]
    k = min(range(n), key=lambda j: abs(ins[j][0] - at))
    print("live before line %d: %d" % (ins[k][0], len(live[k])))
    for r in sorted(live[k]):
        d, u = search(k, r, False), search(k, r, True)
        print("  v%-3d defined at %-24s next used at %-24s %s" % (r, (str(d[:3]) + ("+" if len(d) > 3 else "")) if d else "entry",
                                                                 str(u[:3]) + ("+" if len(u) > 3 else ""), lines[d[0] - 1].strip()[:60] if d else ""))


if __name__ == "__main__":
    main()
