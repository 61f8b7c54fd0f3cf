#!/usr/bin/env python3
"""Static cycle ledger of a kernel's per-position loop, read from the gfx950 assembly the compiler emits.

    python tools/isa_ledger.py                                  # sample_philox_v2_kernel<1,4,1> (the C2 sampler)
    python tools/isa_ledger.py --kernel sample_philox_v2_kernelILi1ELi4ELi2ELb0 --list
    python tools/isa_ledger.py --asm saved.s                    # an assembly file kept earlier (--keep)

The source is compiled device-only to assembly (`hipcc --cuda-device-only -S`: the `.s` that `--save-temps` keeps), whose
block comments carry the compiler's loop nesting.  The per-position loop is the depth-1 loop holding the most `s_barrier`s.
Its hot blocks are those reachable from the loop header without entering a block marked cold in the source (an empty
`asm volatile("; ledger: cold")`, which emits no instruction: the exact fallback of the samplers).  The hot body is cut at
every `s_barrier` into phases, in address order, and every vector instruction is priced with the classes measured on
MI355X (profiles/r03_valu_classes.txt):

  2 cycles  add / sub / and / or / xor / not / mov, right shifts, v_bitop3, compares
  4 cycles  left shifts, mul / mad, every other three-operand form, v_cndmask, min / max, DPP, SDWA, v_mbcnt,
            v_readlane / v_writelane / v_readfirstlane, 64-bit, packed and conversion forms — and any two-operand
            instruction with a scalar-register source

LDS instructions are counted by kind.  Straight-line code counts once whichever way a branch goes (what a wave issues when
its lanes take both sides); the bodies of loops nested in the position loop are listed apart, per iteration, and are not in
the phase totals.  Printed last: VGPRs, SGPRs (and SGPRs spilled to VGPR lanes), scratch, occupancy and static LDS.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_SRC = os.path.join(ROOT, "fl_scaling_sc_ldpc_amd", "csrc", "sampler_v2.hip")
DEFAULT_KERNEL = "sample_philox_v2_kernelILi1ELi4ELi1ELb0"
COLD_MARK = "ledger: cold"

FAST_OPS = {
    "v_add_u32", "v_sub_u32", "v_subrev_u32", "v_and_b32", "v_or_b32", "v_xor_b32", "v_not_b32", "v_mov_b32",
    "v_lshrrev_b32", "v_ashrrev_i32", "v_bitop3_b32", "v_bitop3_b16",
}
SCALAR_SRC = re.compile(r"^-?(s\d+|s\[\d+:\d+\]|vcc(_lo|_hi)?|exec(_lo|_hi)?|m0|ttmp\d+)$")


def price(mnem, operands):
    """Vector cycles of one wave-instruction (2 or 4) by the measured classes."""
    base = re.sub(r"_(e32|e64|dpp|sdwa)$", "", mnem)
    if "_dpp" in mnem or "_sdwa" in mnem or re.search(r"\b(row_\w+|quad_perm|row_mask|bank_mask|dst_sel|src0_sel)", operands):
        return 4
    ops = [o.strip() for o in re.split(r",(?![^\[]*\])", operands)]
    if base.startswith("v_cmp"):
        return 4 if any(SCALAR_SRC.match(o) for o in ops[1:3]) else 2     # ops[0]: the mask written
    if base in FAST_OPS:
        if base in ("v_mov_b32", "v_not_b32"):
            return 2
        return 4 if any(SCALAR_SRC.match(o) for o in ops[1:]) else 2
    return 4


class Block:
    def __init__(self, name, comment):
        self.name, self.insts, self.succ, self.cold = name, [], [], False
        dm = re.findall(r"Depth=(\d+)", comment)
        self.depth = max(int(d) for d in dm) if dm else 0
        hm = re.search(r"in Loop: Header=(BB\w+)", comment)
        self.header = hm.group(1) if hm else (name.lstrip("L") if "Loop Header" in comment else None)
        self.parent = None                      # the depth-1 loop this block belongs to


def compile_asm(src, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-o", out, src]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)


def parse_kernel(asm_text, kernel):
    """The named kernel's basic blocks (instructions, successors, loop nesting) and the compiler's resource figures."""
    lines = asm_text.splitlines()
    labels = [(k, m.group(1)) for k, l in enumerate(lines) for m in [re.match(r"^(_Z\w*):", l)] if m and kernel in m.group(1)]
    if not labels:
        raise SystemExit(f"no kernel matching {kernel!r}")
    if len(labels) > 1:
        raise SystemExit(f"{kernel!r} matches several kernels: {[n for _, n in labels]}")
    i, name = labels[0]
    blocks = [Block("entry", "")]
    k = i + 1
    while k < len(lines) and not lines[k].startswith(".Lfunc_end"):
        l = lines[k]
        k += 1
        m = re.match(r"^(\.LBB\w+|; %bb\.\d+):\s*(;.*)?$", l)
        if m:
            c = m.group(2) or ""
            while k < len(lines) and re.match(r"^\s+;", lines[k]) and COLD_MARK not in lines[k]:
                c += " " + lines[k].strip()     # a block's loop comment runs on over comment-only lines
                k += 1
            blocks.append(Block(m.group(1).replace("; %bb.", "bb.").lstrip("."), c))
            continue
        if COLD_MARK in l:
            blocks[-1].cold = True
            continue
        m = re.match(r"^\s+([a-z_][a-z0-9_]*)\s*(.*?)\s*(;.*)?$", l)
        if m and not l.lstrip().startswith((".", ";")):
            blocks[-1].insts.append((m.group(1), m.group(2)))
    byname = {b.name: b for b in blocks}
    for j, b in enumerate(blocks):
        last = b.insts[-1][0] if b.insts else ""
        for mn, ops in b.insts:
            if mn.startswith(("s_branch", "s_cbranch")):
                b.succ.append(ops.split()[0].lstrip("."))
        if last not in ("s_branch", "s_endpgm", "s_setpc_b64") and j + 1 < len(blocks):
            b.succ.append(blocks[j + 1].name)
        b.succ = [s for s in b.succ if s in byname]
    parent = None
    for b in blocks:                            # blocks of a depth-1 loop lie between its header and its latch
        if b.depth == 1:
            parent = b.header
        b.parent = parent if b.depth >= 1 else None
    res = {}
    for l in lines[i:]:
        m = re.match(r"^;\s*(NumVgprs|TotalNumSgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\d+)", l)
        if m and m.group(1) not in res:
            res[m.group(1)] = int(m.group(2))
        if len(res) == 5:
            break
    for key, field in (("SgprSpills", "sgpr_spill_count"), ("VgprSpills", "vgpr_spill_count")):
        m = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:\s+\.[^\n]*\n)*?\s+\." + field + r":\s+(\d+)", asm_text)
        res[key] = int(m.group(1)) if m else -1
    return name, blocks, res


def position_loop(blocks):
    """Header of the depth-1 loop with the most s_barriers."""
    bars = collections.Counter(b.parent for b in blocks if b.parent for mn, _ in b.insts if mn == "s_barrier")
    if not bars:
        raise SystemExit("no loop with a barrier in this kernel")
    return bars.most_common(1)[0][0]


def hot_blocks(blocks, loop):
    byname = {b.name: b for b in blocks}
    start = byname["L" + loop]
    seen, todo = {start.name}, [start]
    while todo:
        b = todo.pop()
        for s in b.succ:
            t = byname[s]
            if t.name not in seen and t.parent == loop and not t.cold:
                seen.add(t.name)
                todo.append(t)
    return seen


def new_phase():
    return dict(n=0, vfast=0, vslow=0, cyc=0, lds=collections.Counter(), salu=0, vmem=0, inner=collections.OrderedDict())


def ledger(blocks, loop, listing=None):
    hot = hot_blocks(blocks, loop)
    phases = [new_phase()]
    for b in blocks:
        if b.name not in hot:
            continue
        for mn, ops in b.insts:
            ph = phases[-1]
            c = price(mn, ops) if mn.startswith("v_") else None
            if listing is not None:
                listing.append(f"{len(phases) - 1:>2} {b.name:>9} d{b.depth} {'' if c is None else c:>2}  {mn} {ops}")
            if mn == "s_barrier":
                phases.append(new_phase())
                continue
            if b.depth >= 2:
                d = ph["inner"].setdefault(b.header, collections.Counter())
                if c is not None:
                    d["v"] += 1
                    d["cyc"] += c
                elif mn.startswith("ds_"):
                    d["lds"] += 1
                continue
            if c is not None:
                ph["n"] += 1
                ph["cyc"] += c
                ph["vfast" if c == 2 else "vslow"] += 1
            elif mn.startswith("ds_"):
                ph["lds"][mn] += 1
            elif mn.startswith(("global_", "buffer_", "flat_")):
                ph["vmem"] += 1
            elif mn.startswith("s_"):
                ph["salu"] += 1
    # the code before the first barrier continues the code after the last one (the back edge joins them)
    if len(phases) > 1:
        a, b = phases[-1], phases.pop(0)
        for key in ("n", "vfast", "vslow", "cyc", "salu", "vmem"):
            a[key] += b[key]
        a["lds"].update(b["lds"])
        for h, d in b["inner"].items():
            a["inner"].setdefault(h, collections.Counter()).update(d)
    return phases


def report(name, blocks, res, out=sys.stdout, listing=False):
    loop = position_loop(blocks)
    lst = [] if listing else None
    phases = ledger(blocks, loop, lst)
    if listing:
        print("phase block depth cycles instruction (listing phase 0 is joined to the last phase below)", file=out)
        print("\n".join(lst), file=out)
    ncold = sum(1 for b in blocks if b.parent == loop and b.cold)
    print(f"kernel {name}", file=out)
    print(f"per-position loop: header {loop}, {len(phases)} phases cut at s_barrier, {ncold} cold region(s) left out", file=out)
    print(f"{'phase':>5} {'VALU':>5} {'2-cyc':>6} {'4-cyc':>6} {'cycles':>7} {'SALU':>5} {'VMEM':>5} {'LDS':>4}  LDS by kind",
          file=out)
    tot, lds_tot = collections.Counter(), collections.Counter()
    for i, ph in enumerate(phases):
        kinds = " ".join(f"{k}:{v}" for k, v in sorted(ph["lds"].items()))
        print(f"{i:>5} {ph['n']:>5} {ph['vfast']:>6} {ph['vslow']:>6} {ph['cyc']:>7} {ph['salu']:>5} {ph['vmem']:>5} "
              f"{sum(ph['lds'].values()):>4}  {kinds}", file=out)
        for h, d in ph["inner"].items():
            print(f"{'':>5}   inner loop {h}: {d['v']} VALU, {d['cyc']} cycles, {d['lds']} LDS per iteration", file=out)
        for k in ("n", "vfast", "vslow", "cyc", "salu", "vmem"):
            tot[k] += ph[k]
        lds_tot.update(ph["lds"])
    print(f"{'total':>5} {tot['n']:>5} {tot['vfast']:>6} {tot['vslow']:>6} {tot['cyc']:>7} {tot['salu']:>5} {tot['vmem']:>5} "
          f"{sum(lds_tot.values()):>4}  (inner loops not included)", file=out)
    print(f"resources: VGPRs {res.get('NumVgprs')} SGPRs {res.get('TotalNumSgprs')} (spilled to VGPR lanes: "
          f"{res.get('SgprSpills')}) VGPR spills {res.get('VgprSpills')} scratch {res.get('ScratchSize')} B, "
          f"occupancy {res.get('Occupancy')} waves/SIMD, static LDS {res.get('LDSByteSize', 0)} B", file=out)
    return dict(phases=phases, total=tot, lds=lds_tot, res=res, loop=loop)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--src", default=DEFAULT_SRC, help="HIP source to compile (ignored with --asm)")
    ap.add_argument("--asm", help="read this device assembly instead of compiling")
    ap.add_argument("--kernel", default=DEFAULT_KERNEL, help="substring of the mangled kernel name")
    ap.add_argument("--keep", help="also write the assembly here")
    ap.add_argument("--list", action="store_true", help="print the hot loop's instructions with phase and price first")
    args = ap.parse_args(argv)
    if args.asm:
        text = open(args.asm).read()
    else:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "k.s")
            compile_asm(args.src, out)
            text = open(out).read()
        if args.keep:
            open(args.keep, "w").write(text)
    name, blocks, res = parse_kernel(text, args.kernel)
    report(name, blocks, res, listing=args.list)


if __name__ == "__main__":
    main()
