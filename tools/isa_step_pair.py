"""Instruction count and mix of the Jacobi step pair (the loop with the 114 DPP moves) in the ISA of the production wave kernel.
Usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -S --cuda-device-only scale-letkf_amd/csrc/letkf_wave.hip -o /tmp/wave.s; python tools/isa_step_pair.py /tmp/wave.s
(or the assembly the Makefile leaves beside the objects: scale-letkf_amd/lib/obj/letkf_wave-hip-amdgcn-amd-amdhsa-gfx950.s)
The loop is found by tools/isa_point_census.py's selector (step_pair there), the one rule of both tools."""
import os
import sys
from collections import Counter
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_point_census
def steppair(path, kern="_ZN5letkf17letkf_wave_kernelILi50ELi11ELb0ELi1ELi0EEEvNS_9PointArgsE:"):
    """(instructions, Counter of opcodes, the instructions as lines) of the step pair of `kern` in the assembly at `path`"""
    ins, labels = isa_point_census.instructions(isa_point_census.function_lines(path, kern.rstrip(":")))
    span = isa_point_census.step_pair(ins, isa_point_census.loops(ins, labels))
    if span is None:
        raise SystemExit(f"no loop with DPP moves in {kern} of {path}")
    body = ins[span[0]:span[1] + 1]
    return len(body), Counter(op for op, _ in body), [f"\t{op} {args}".rstrip() for op, args in body]
if __name__=="__main__":
    for p in sys.argv[1:]:
        n,c,b=steppair(p)
        print(p,n,c.most_common(16))
