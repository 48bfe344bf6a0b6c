#!/usr/bin/env python3
"""GPU: A/B of two builds of liblsnf_flow.so in one job (alternating child processes, LSNF_LIB_PATH): kernel-only time of the
headline forward (and optionally other entry points) per math mode.   usage: ab_libs.py libA.so libB.so [rounds]"""
import os
import sys

import ab_harness

CHILD = r'''
import os, sys, torch
import bench, lsnf_amd
F = lsnf_amd.flow
dev = torch.device("cuda:0")
plan = lsnf_amd.prepare([t.to(dev) for t in bench.synth_weights(1)], bench.NZ, bench.WIDTH, bench.DEPTH)
F.set_small_batch_max(0)
z = torch.randn(65536, bench.NZ, generator=torch.Generator().manual_seed(1234)).to(dev)
outs = (torch.empty_like(z), torch.empty(z.shape[0], device=dev), torch.empty(z.shape[0], device=dev))
def t_us(fn, n=400):
    for _ in range(600): fn()
    torch.cuda.synchronize()
    return windows(fn, n, 1)[0]
res = []
for name, mode in (("fwd3b", getattr(F, "MATH_BF16X3_PHASED", F.MATH_BF16X3)), ("fwd3q", F.MATH_BF16X3)):
    F.set_math_mode(mode)
    res.append(f"{name} {t_us(lambda: lsnf_amd.forward(plan, z, out=outs)):.2f}")
F.set_math_mode(F.MATH_BF16X3)
emit("  ".join(res))
'''


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    rounds = int(argv[2]) if len(argv) > 2 else 2
    res = ab_harness.run(CHILD, [(lib, lib, {}) for lib in argv[:2]], rounds, timeout=280,
                         ok=lambda lib, r, line: f"{os.path.basename(lib):24s} {line}")
    return 1 if res is None else 0


if __name__ == "__main__":
    sys.exit(main())
