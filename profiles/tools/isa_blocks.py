#!/usr/bin/env python3
"""profiles/tools/isa_blocks.py [kernel-substring] [--hist] [--min-depth N] [--asm FILE] [-Dflags...] -- basic blocks of one fused-pass kernel
(default k_fusedPass<true,0,0>) with their VALU / SALU / LDS / SMEM / VMEM instruction counts and the loop nest the compiler's comments give
them: the static half of "where do the instructions go" (profiles/trip_counts.py is the dynamic half).  Compiles pt_kernels_fused.hip to
assembly with the product flags (+ any -D given), or reads an assembly file made that way (--asm).
--hist: under every block its opcode histogram of the non-arithmetic VALU instructions (moves, selects, compares, lane reads / writes) and the
s_nop padding -- v_mov_b32 split by what it moves (:vgpr a copy, :sgpr a scalar operand, :const an initialisation) -- and at the end the same
histogram summed per loop depth, the out-of-line blocks (rare branches, marked *) apart.  --min-depth N: only blocks at loop depth >= N are listed."""
import os, re, subprocess, sys
here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "2015-raytracing_amd", "csrc")
args = sys.argv[1:]
want = args.pop(0) if args and not args[0].startswith("-") else "k_fusedPassILb1ELi0ELi0ELi0ELb0ELb0ELb0E"   # <FAST, GRIDS 0, WAVES 0, MULTI 0, SEG, EVERY, GUIDES all false>: the whole name, a prefix matches the multi-pass instances first
hist = "--hist" in args
if hist: args.remove("--hist")
min_depth = 0
if "--min-depth" in args:
    at = args.index("--min-depth")
    min_depth = int(args[at + 1])
    del args[at:at + 2]
asm = "/tmp/isa_blocks.s"
if "--asm" in args:
    at = args.index("--asm")
    asm = args[at + 1]
    del args[at:at + 2]
else:
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "-S", "--cuda-device-only", "pt_kernels_fused.hip", "-o", asm] + args
    subprocess.run(cmd, cwd=here, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
lines = open(asm).read().splitlines()
start = next(i for i, l in enumerate(lines) if re.match(r"^_ZN2pt11" + want + r"\w*:", l))
end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))   # (a kernel has several s_endpgm: its early returns)
body = lines[start:end + 1]
blocks, cur = [], {"label": "entry", "depth": 0, "ins": [], "line": 0}
for n, l in enumerate(body):
    m = re.match(r"^(\.LBB\d+_\d+):", l)
    if m:
        blocks.append(cur)
        cur = {"label": m.group(1), "depth": 0, "ins": [], "line": n}
        m2 = re.search(r"Depth=(\d+)", l)   # the loop comment may sit on the label's own line (".LBB49_98:   ; in Loop: Header=BB49_49 Depth=1")
        if m2: cur["depth"] = int(m2.group(1))
        continue
    m = re.search(r"Depth[= ](\d+)", l)
    if m and ("Loop Header" in l or "in Loop" in l):
        cur["depth"] = max(cur["depth"], int(m.group(1)))
    m = re.match(r"^; %bb\.(\d+):", l)
    if m:
        blocks.append(cur)
        cur = {"label": "bb." + m.group(1), "depth": 0, "ins": [], "line": n}
        m2 = re.search(r"Depth=(\d+)", l)
        if m2: cur["depth"] = int(m2.group(1))
        continue
    t = l.strip()
    if t and not t.startswith(";") and not t.startswith("."):
        op = t.split()[0]
        if op.startswith("v_mov_b32_e"):   # what is moved: another VGPR (a phi copy), an SGPR (a scalar operand no VOP2 slot took), a constant (an initialisation)
            src = t.split(";")[0].split(",")[-1].strip()
            op = "v_mov_b32" + (":vgpr" if src.startswith("v") and not src.startswith("vcc") else ":sgpr" if src.startswith(("s", "vcc", "exec", "ttmp", "m0")) else ":const")
        cur["ins"].append(op)
        if op == "s_cbranch_execnz": cur.setdefault("rare_to", []).append(t.split()[1])
blocks.append(cur)
# Out of line: the compiler lays a branch it expects not to be taken (__builtin_expect, a slow path of the math library) out after the code that
# follows it and enters it by s_cbranch_execnz; the run of blocks from such a target to the s_branch that leads back is marked '*' and summed
# apart -- its instructions are in the static totals and (nearly) never issue.
rare_targets = {x for b in blocks for x in b.get("rare_to", [])}
inside = False
for b in blocks:
    if b["label"] in rare_targets: inside = True
    b["rare"] = inside
    if inside and b["ins"] and b["ins"][-1] == "s_branch": inside = False
MISC = ("v_cmp", "v_cndmask", "v_mov", "v_readfirstlane", "v_readlane", "v_writelane", "v_accvgpr")
def cls(op):
    if op.startswith(MISC): return "vmisc"
    if op.startswith("v_"): return "valu"
    if op.startswith("ds_"): return "lds"
    if op.startswith(("s_load", "s_buffer_load")): return "smem"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")): return "vmem"
    if op.startswith("s_"): return "salu"
    return "other"
def audited(op):   # what --hist itemises: every vmisc opcode (compares folded to v_cmp / v_cmpx), min / max / med3, and the s_nop padding
    if op.startswith("v_cmpx"): return "v_cmpx"
    if op.startswith("v_cmp"): return "v_cmp"
    if op.startswith(MISC) or op.startswith(("v_min", "v_max", "v_med3")) or op == "s_nop": return re.sub(r"_e(32|64)$", "", op)
    return None
tot, by_depth = {}, {}
print(f"{'line':>5s} {'block':12s} depth  valu vmisc salu lds smem vmem   (* = out of line)")
for b in blocks:
    c, h = {}, {}
    for op in b["ins"]:
        c[cls(op)] = c.get(cls(op), 0) + 1
        tot[cls(op)] = tot.get(cls(op), 0) + 1
        a = audited(op)
        if a:
            h[a] = h.get(a, 0) + 1
            d = by_depth.setdefault((b["depth"], b["rare"]), {})
            d[a] = d.get(a, 0) + 1
    if not b["ins"] or b["depth"] < min_depth: continue
    print(f"{b['line']:5d} {b['label']:12s} {b['depth']:5d} {c.get('valu',0):5d} {c.get('vmisc',0):5d} {c.get('salu',0):4d} {c.get('lds',0):3d} {c.get('smem',0):4d} {c.get('vmem',0):4d}" + (" *" if b["rare"] else ""))
    if hist and h:
        print("      " + "  ".join(f"{k} {v}" for k, v in sorted(h.items())))
print("total", tot, "lines", len(body))
if hist:
    for d, rare in sorted(by_depth):
        print(f"depth {d}{' out of line' if rare else ''}: " + "  ".join(f"{k} {v}" for k, v in sorted(by_depth[(d, rare)].items())))
