"""Instruction mix of the flying loop of the role kernel, read from a gfx950 compile (no GPU needed).

    python tools/loop_mix.py [--kernel MANGLED_NAME] [--loop N] [--asm-dir DIR] [--no-regs]

Compiles mcfost_amd/csrc/kern_roles.hip (and kern_tail.hip, for the register report) with the library's flags plus
--cuda-device-only -S into a temporary directory, cuts out the function of one instantiation (default: the Pascucci
headline's k_thermal_roles<false,false,false,true,false,true>: the padded cell key) and finds its flying loop: the innermost natural loop whose body
holds the LDS deposit (ds_add_f64).  The loop's blocks are split into the common path and the rare blocks, and each part
is counted by kind.  Rare are the blocks that hold the stop's division (v_div_scale_f64), the default-real zj fallback
(v_cvt_f32_f64) or the runaway store (global_store), and every block that one of these dominates, unless it also
dominates the loop's latch (a region without a skip branch is part of the straight line): the stop's own deposit and
commit sit in blocks of their own behind its division, while the deposit of the lanes that go on is in the common path.
Both sides of a divergent if/else count: a wave runs both.
A third column, "cold", counts the blocks without a marker that the compiler laid out of line: entered only by a taken
s_cbranch_execnz and left by s_branch, which is where it puts what __builtin_expect calls unlikely.  In the padded kernels
without a dark zone that is the leave test behind its guard (fly_leave_2d, about once per packet); the guard itself -- two
compares, two mask operations and the region's s_and_saveexec -- stays in the common path.

What the counts mean:
  VALU        every v_* instruction (v_readlane / v_writelane included)
  SALU        every s_* instruction except s_waitcnt, s_nop and the branches
  FP64        v_* FP64 arithmetic: add, mul, fma/fmac, min/max, floor, rsq/rcp, div_* (not compares, not conversions)
  cndmask     v_cndmask_b32
  literal     v_mov_b32 of a literal constant (0x...) and v_bfrev_b32: constants rematerialised each iteration
  branches    s_cbranch_* and s_branch
  regions     exec-mask branch regions (s_and_saveexec_b64 / s_andn2_saveexec_b64 / s_or_saveexec_b64)
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "mcfost_amd", "csrc")

PASCUCCI = "_ZN5mcgpu15k_thermal_rolesILb0ELb0ELb0ELb1ELb0ELb1EEEvNS_8DevModelENS_7RunArgsEiiiiii"
REG_REPORT = [
    ("kern_roles.hip", PASCUCCI, "k_thermal_roles<false,false,false,true,false,true> (Pascucci)"),
    ("kern_tail.hip", "_ZN5mcgpu20k_thermal_roles_tailILb1ELb0ELb1ELb0ELb0EEEvNS_8DevModelENS_7RunArgsEiiiiii",
     "k_thermal_roles_tail<true,false,true,false,false> (ref4.1 2D)"),
    ("kern_tail.hip", "_ZN5mcgpu6k_tailILb0ELb1ELb0ELb0EEEvNS_8DevModelENS_7RunArgsEPKvPKjPj",
     "k_tail<false,true,false,false>"),
]
RARE_MARKERS = ("v_div_scale_f64", "v_cvt_f32_f64", "global_store")
FP64_OPS = re.compile(r"^v_(add|mul|fma|fmac|min|max|floor|rsq|rcp|div_scale|div_fmas|div_fixup|ldexp|fract|trunc|ceil|sqrt)_f64")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]*)\b")
BRANCH = re.compile(r"^\s+(s_cbranch_\w+|s_branch)\s+(\.LBB\w+)")


def compile_asm(unit, out_dir):
    import __graft_entry__ as g
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = os.path.join(out_dir, os.path.splitext(unit)[0] + ".s")
    if not os.path.exists(out):
        subprocess.run([hipcc] + g.HIPCC_COMPILE + ["--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, unit)],
                       check=True, stderr=subprocess.DEVNULL)
    return out


def function_text(asm_lines, name):
    starts = [k for k, l in enumerate(asm_lines) if l.startswith(name + ":")]
    if not starts:
        raise SystemExit("no function %s in the assembly" % name)
    i = starts[0]
    j = next(k for k in range(i, len(asm_lines)) if asm_lines[k].startswith(".Lfunc_end"))
    return asm_lines[i:j], asm_lines[j:]


def kernel_resources(tail_lines, name):
    """VGPRs (arch + accumulation) and private segment (scratch) size from the kernel descriptor that follows."""
    vgpr = scratch = None
    for l in tail_lines[:100]:
        m = re.match(r"^; TotalNumVgprs: (\d+)", l)
        if m and vgpr is None:
            vgpr = int(m.group(1))
        m = re.match(r"^; ScratchSize: (\d+)", l)
        if m and scratch is None:
            scratch = int(m.group(1))
    return vgpr, scratch


def basic_blocks(body):
    starts = {0}
    for k, l in enumerate(body):
        if re.match(r"^\.LBB\w+:", l):
            starts.add(k)
        if re.match(r"^\s+(s_cbranch_\w+|s_branch|s_endpgm|s_setpc_b64)\b", l) and k + 1 < len(body):
            starts.add(k + 1)
    starts = sorted(starts)
    blocks = [(s, starts[i + 1] if i + 1 < len(starts) else len(body)) for i, s in enumerate(starts)]
    label = {}
    for i, (s, _) in enumerate(blocks):
        m = re.match(r"^(\.LBB\w+):", body[s])
        if m:
            label[m.group(1)] = i
    succ = [set() for _ in blocks]
    for i, (s, e) in enumerate(blocks):
        last = next((body[k] for k in range(e - 1, s - 1, -1) if INSN.match(body[k])), None)
        falls = True
        if last is not None:
            m = BRANCH.match(last)
            if m:
                succ[i].add(label[m.group(2)])
                falls = m.group(1) != "s_branch"
            if re.match(r"^\s+(s_endpgm|s_setpc_b64)\b", last):
                falls = False
        if falls and i + 1 < len(blocks):
            succ[i].add(i + 1)
    return blocks, succ


def natural_loops(n, succ):
    pred = [set() for _ in range(n)]
    for i in range(n):
        for j in succ[i]:
            pred[j].add(i)
    reach, stack = {0}, [0]
    while stack:
        for y in succ[stack.pop()]:
            if y not in reach:
                reach.add(y)
                stack.append(y)
    dom = {i: set(reach) for i in reach}
    dom[0] = {0}
    order = sorted(reach)
    changed = True
    while changed:
        changed = False
        for i in order[1:]:
            ps = [dom[p] for p in pred[i] if p in reach]
            d = (set.intersection(*ps) if ps else set()) | {i}
            if d != dom[i]:
                dom[i], changed = d, True
    loops = []
    for t in reach:
        for h in succ[t]:
            if h in reach and h in dom[t]:
                body, stack = {h, t}, [t]
                while stack:
                    x = stack.pop()
                    if x == h:
                        continue
                    for p in pred[x]:
                        if p not in body and p in reach:
                            body.add(p)
                            stack.append(p)
                loops.append((h, body))
    return loops, dom


def mix(lines):
    c = dict(VALU=0, SALU=0, FP64=0, cndmask=0, literal=0, branches=0, regions=0, LDS=0, VMEM=0)
    for l in lines:
        m = INSN.match(l)
        if not m:
            continue
        op = m.group(1)
        if op.startswith("v_"):
            c["VALU"] += 1
            if FP64_OPS.match(op):
                c["FP64"] += 1
            if op.startswith("v_cndmask_b32"):
                c["cndmask"] += 1
            if (op.startswith("v_mov_b32") and re.search(r",\s*0x[0-9a-f]+\s*$", l)) or op.startswith("v_bfrev_b32"):
                c["literal"] += 1
        elif op.startswith("s_"):
            if op.startswith(("s_cbranch", "s_branch")):
                c["branches"] += 1
            elif not op.startswith(("s_waitcnt", "s_nop")):
                c["SALU"] += 1
            if re.match(r"s_(and|andn2|or)_saveexec_b64", op):
                c["regions"] += 1
        elif op.startswith("ds_"):
            c["LDS"] += 1
        elif op.startswith(("global_", "flat_", "buffer_", "scratch_")):
            c["VMEM"] += 1
    return c


def flying_loop(body, which=0):
    blocks, succ = basic_blocks(body)
    loops, dom = natural_loops(len(blocks), succ)
    dep_blocks = [i for i, (s, e) in enumerate(blocks) if any(re.match(r"^\s+ds_add_f64\b", body[k]) for k in range(s, e))]
    if not dep_blocks:
        raise SystemExit("no LDS deposit (ds_add_f64) in this function")
    found = []
    for d in dep_blocks:
        cands = sorted((l for l in loops if d in l[1]), key=lambda l: len(l[1]))
        if cands and cands[0] not in found:
            found.append(cands[0])
    found.sort(key=lambda l: blocks[l[0]][0])
    h, loop = found[which]
    has = lambda i, mk: any(mk in l for l in body[blocks[i][0]:blocks[i][1]])
    latches = [t for t in loop if h in succ[t]]
    marked = {i for i in loop if any(has(i, mk) for mk in RARE_MARKERS)}
    side = {i for i in marked if not any(i in dom[t] for t in latches)}   # (these take what they dominate with them)
    def last_insn(i):
        return next((body[k] for k in range(blocks[i][1] - 1, blocks[i][0] - 1, -1) if INSN.match(body[k])), "")

    def out_of_line(i):
        preds = [p for p in loop if i in succ[p]]
        name = body[blocks[i][0]].split(":")[0]
        return bool(preds) and re.match(r"^\s+s_branch\b", last_insn(i)) is not None and \
            all(re.match(r"^\s+s_cbranch_execnz\s+" + re.escape(name) + r"\s*$", last_insn(p)) for p in preds)

    common, rare, cold = [], [], []
    for i in sorted(loop):
        s, e = blocks[i]
        if i in marked or any(j in dom[i] for j in side):
            rare.extend(body[s:e])
        elif i != h and out_of_line(i):
            cold.extend(body[s:e])
        else:
            common.extend(body[s:e])
    return common, rare, cold, len(found), body[blocks[h][0]].split(":")[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", default=PASCUCCI, help="mangled name of the instantiation (kern_roles.hip)")
    ap.add_argument("--loop", type=int, default=0, help="which loop with a deposit, in code order (0: the flying waves')")
    ap.add_argument("--asm-dir", default=None, help="directory of kern_roles.s / kern_tail.s (reused, else compiled)")
    ap.add_argument("--no-regs", action="store_true", help="skip the register report (and the kern_tail.hip compile)")
    a = ap.parse_args()
    tmp = a.asm_dir or tempfile.mkdtemp(prefix="loop_mix_")
    os.makedirs(tmp, exist_ok=True)
    asm = open(compile_asm("kern_roles.hip", tmp)).read().split("\n")
    body, _ = function_text(asm, a.kernel)
    common, rare, cold, n_loops, header = flying_loop(body, a.loop)
    cm, rm, km = mix(common), mix(rare), mix(cold)
    print("flying loop of %s\n  (loop %d of %d with an LDS deposit, header %s)" % (a.kernel, a.loop, n_loops, header))
    keys = ["VALU", "FP64", "cndmask", "literal", "SALU", "branches", "regions", "LDS", "VMEM"]
    print("  %-12s %8s %8s %8s" % ("per iteration", "common", "rare", "cold"))
    for k in keys:
        print("  %-12s %8d %8d %8d" % (k, cm[k], rm[k], km[k]))
    if a.no_regs:
        return
    print("registers (VGPRs incl. AGPRs, scratch bytes per lane):")
    for unit, name, label in REG_REPORT:
        lines = open(compile_asm(unit, tmp)).read().split("\n")
        _, tail = function_text(lines, name)
        v, s = kernel_resources(tail, name)
        print("  %-58s VGPR %4s  scratch %4s" % (label, v, s))


if __name__ == "__main__":
    main()
