#!/usr/bin/env python3
"""Census of one kernel instantiation in a unit's kept device assembly: where the vector issue slots outside the Jacobi step
pair go, and in particular the lane traffic of spilled scalars (v_writelane_b32 in the prologue, v_readlane_b32 at every use).

Usage: python tools/isa_point_census.py [UNIT.s] [--kernel MANGLED_NAME]
  (default: scale-letkf_amd/lib/obj/letkf_wave-hip-amdgcn-amd-amdhsa-gfx950.s, the assembly the Makefile keeps beside the
   objects, and letkf_wave_kernel<50, 11, false, 1, 0>)

Prints the loop map (every backward branch gives a loop [target label, branch]; nested loops are indented), per loop and for the
whole function the counts of COUNTED below, the registers v_writelane_b32 writes, the lane reads by region of the function
(cut at its largest loops), and what the lane reads feed: the next instruction that uses the destination scalar."""
import argparse
import os
import re
from collections import Counter

KERNEL = "_ZN5letkf17letkf_wave_kernelILi50ELi11ELb0ELi1ELi0EEEvNS_9PointArgsE"
DEFAULT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scale-letkf_amd", "lib", "obj",
                       "letkf_wave-hip-amdgcn-amd-amdhsa-gfx950.s")
COUNTED = ("valu", "mfma", "v_readlane_b32", "v_writelane_b32", "s_nop", "v_cndmask_b32", "v_div_fixup_f64", "scratch")


def function_lines(path, kernel=KERNEL):
    """The lines of `kernel` in the assembly at `path`, from its label to its s_endpgm."""
    out, inside = [], False
    with open(path) as f:
        for line in f:
            if line.startswith(kernel + ":"):
                inside = True
            elif inside:
                out.append(line.rstrip("\n"))
                if line.strip().startswith("s_endpgm"):
                    return out
    raise SystemExit(f"{kernel} not found in {path}")


def instructions(lines):
    """[(opcode, operand text)] of the function and {label: index of the first instruction behind it}."""
    ins, labels = [], {}
    for l in lines:
        s = l.split(";")[0].strip()
        if not s:
            continue
        if s.endswith(":"):
            labels[s[:-1]] = len(ins)
        elif not s.startswith("."):
            op, _, rest = s.partition(" ")
            op, _, rest2 = op.partition("\t")
            ins.append((op, (rest2 + " " + rest).strip()))
    return ins, labels


def count(ins):
    c = Counter({key: 0 for key in COUNTED})
    c["all"] = len(ins)
    for op, _ in ins:
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
        if op.startswith("scratch_"):
            c["scratch"] += 1
        for key in ("v_readlane_b32", "v_writelane_b32", "s_nop", "v_cndmask_b32", "v_div_fixup_f64"):
            if op == key or op.startswith(key + "_e"):
                c[key] += 1
    return c


def loops(ins, labels):
    """[(first, last)] instruction indices of every loop, outermost first; one per backward branch."""
    found = set()
    for i, (op, args) in enumerate(ins):
        if op.startswith("s_cbranch") or op == "s_branch":
            t = labels.get(args.split()[-1])
            if t is not None and t <= i:
                found.add((t, i))
    return sorted(found, key=lambda ab: (ab[0], -ab[1]))


def step_pair(ins, lps):
    """The Jacobi step pair, (first, last) or None: the backward branch whose span is densest in DPP moves, among those with
    fewer than 200 of them.  (A cold block that hipcc lays out behind the point loop and that jumps back into it is a backward
    branch too, thousands of instructions long, with the DPP moves of every reduction it spans.)  The one selector of the
    tools: tools/isa_step_pair.py calls it."""
    best, span = 0.0, None
    for a, b in lps:
        nd = sum(op == "v_mov_b32_dpp" for op, _ in ins[a:b + 1])
        if 0 < nd < 200 and nd / (b - a + 1) > best:
            best, span = nd / (b - a + 1), (a, b)
    return span


def gram_tile_loop(ins, lps):
    """The Gram's observation-tile loop: the innermost loop with matrix instructions in front of the step pair."""
    sp = step_pair(ins, lps)
    best = None
    for a, b in lps:
        if (sp is None or b < sp[0]) and any(op.startswith("v_mfma") for op, _ in ins[a:b + 1]):
            if best is None or (b - a) < (best[1] - best[0]):
                best = (a, b)
    return best


def point_loop(ins, lps):
    """The point loop: the longest loop of the function."""
    return max(lps, key=lambda ab: ab[1] - ab[0]) if lps else None


def sregs(text):
    """The scalar registers an operand text names, ranges expanded."""
    out = set()
    for m in re.finditer(r"\bs\[(\d+):(\d+)\]|\bs(\d+)\b|\b(vcc|exec)(_lo|_hi)?\b", text):
        if m.group(1):
            out.update(f"s{n}" for n in range(int(m.group(1)), int(m.group(2)) + 1))
        elif m.group(3):
            out.add("s" + m.group(3))
        else:
            out.add(m.group(4) + (m.group(5) or ""))
    return out


def readlane_consumers(ins):
    """Counter of the opcode that first uses the scalar a v_readlane_b32 wrote (or 'dead/redefined', '(none)')."""
    c = Counter()
    for i, (op, args) in enumerate(ins):
        if op != "v_readlane_b32":
            continue
        dst = args.split(",")[0].strip()
        who = "(none)"
        for op2, args2 in ins[i + 1:i + 400]:
            parts = args2.split(",")
            # stores, compares into exec and branches have no register destination; everything else writes its first operand
            srcs = args2 if (op2.startswith(("s_cmp", "s_cbranch", "scratch_store", "global_store", "ds_write", "s_waitcnt")))\
                else ",".join(parts[1:])
            full = srcs if not op2.endswith("saveexec_b64") else args2
            if dst in sregs(full):
                who = op2
                break
            if dst in sregs(parts[0]):
                who = "dead/redefined"
                break
        c[who] += 1
    return c


def writelane_registers(ins):
    return sorted({args.split(",")[0].strip() for op, args in ins if op == "v_writelane_b32"}, key=lambda r: int(r[1:]))


def census(path=DEFAULT, kernel=KERNEL):
    ins, labels = instructions(function_lines(path, kernel))
    lps = loops(ins, labels)
    sp, gt, pl = step_pair(ins, lps), gram_tile_loop(ins, lps), point_loop(ins, lps)
    sub = lambda ab: count(ins[ab[0]:ab[1] + 1]) if ab else None
    return {"function": count(ins), "loops": [(a, b, count(ins[a:b + 1])) for a, b in lps], "step_pair": sub(sp),
            "gram_tile_loop": sub(gt), "point_loop": sub(pl), "writelane_registers": writelane_registers(ins),
            "readlane_consumers": readlane_consumers(ins), "spans": {"step_pair": sp, "gram_tile_loop": gt, "point_loop": pl},
            "prologue": count(ins[:pl[0]]) if pl else None, "ins": ins}


def fmt(c):
    return " ".join(f"{key}={c[key]}" for key in ("all",) + COUNTED)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("unit", nargs="?", default=DEFAULT)
    ap.add_argument("--kernel", default=KERNEL)
    a = ap.parse_args()
    r = census(a.unit, a.kernel)
    print("function      ", fmt(r["function"]))
    print("prologue      ", fmt(r["prologue"]))
    for name in ("point_loop", "gram_tile_loop", "step_pair"):
        print(f"{name:14s}", r["spans"][name], fmt(r[name]) if r[name] else "-")
    print("loop map (first, last instruction; nesting by indent):")
    stack = []
    for lo, hi, c in r["loops"]:
        while stack and lo > stack[-1]:
            stack.pop()
        print("  " * (1 + len(stack)) + f"[{lo}, {hi}] " + fmt(c))
        stack.append(hi)
    # lane reads by region: the gaps between the top-level loops of the point loop
    pl = r["spans"]["point_loop"]
    if pl:
        inner = [(lo, hi) for lo, hi, _ in r["loops"] if pl[0] <= lo and hi <= pl[1] and (lo, hi) != pl]
        top = [ab for ab in inner if not any(o[0] <= ab[0] and ab[1] <= o[1] and o != ab for o in inner)]
        cuts, at = [], pl[0]
        for lo, hi in top:
            cuts.append((f"straight [{at}, {lo})", at, lo))
            cuts.append((f"loop     [{lo}, {hi}]", lo, hi + 1))
            at = hi + 1
        cuts.append((f"straight [{at}, {pl[1]}]", at, pl[1] + 1))
        print("v_readlane_b32 / all instructions by region of the point loop:")
        for name, lo, hi in cuts:
            c = count(r["ins"][lo:hi])
            if c["all"]:
                print(f"  {name:28s} {c['v_readlane_b32']:5d} / {c['all']}")
    print("registers written by v_writelane_b32:", len(r["writelane_registers"]), " ".join(r["writelane_registers"]))
    print("what the lane reads feed (next use of the scalar):")
    for op, n in r["readlane_consumers"].most_common(24):
        print(f"  {n:5d} {op}")
