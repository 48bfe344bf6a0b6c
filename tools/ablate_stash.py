"""GPU: time of the forward with stash at B = 65 536 for each library given (the variants tools/ablate_stash.sh builds), one child
process per library:   python tools/ablate_stash.py _ablate/s_0.so _ablate/s_1.so ..."""
import sys

import ab_harness

CHILD = r'''
import os, sys, torch
import bench, lsnf_amd
F = lsnf_amd.flow
dev = torch.device("cuda:0")
F.set_small_batch_max(0)
w = bench.synth_weights(1)
plan = lsnf_amd.prepare([t.to(dev) for t in w], bench.NZ, bench.WIDTH, bench.DEPTH)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
zd = torch.randn(B, bench.NZ, device=dev)
act = F.new_act_saved(plan, B, dev)
outs = (torch.empty_like(zd), torch.empty(B, device=dev), torch.empty(B, device=dev))
saved = torch.empty(bench.DEPTH - 1, B, bench.NZ, device=dev)
def t_us(fn, n=300):
    for _ in range(300): fn()
    torch.cuda.synchronize()
    return sorted(windows(fn, n, 7))[3]
a = t_us(lambda: lsnf_amd.forward(plan, zd, out=outs))
b = t_us(lambda: lsnf_amd.forward(plan, zd, out=outs, act_saved=act, z_saved_out=saved))
gg = torch.randn(B, bench.NZ, device=dev); nn_ = torch.randn(B, bench.NZ, device=dev)
c = t_us(lambda: F.langevin_step(plan, zd, gg, nn_, 0.1, reuse_buffers=True))
emit(f"B={B} forward {a:6.1f} us  forward+stash {b:6.1f} us  Langevin step {c:6.1f} us")
'''


def main(argv=None):
    libs = sys.argv[1:] if argv is None else argv
    res = ab_harness.run(CHILD, [(lib, lib, {}) for lib in libs], timeout=120, ok=lambda lib, r, line: f"{lib}: {line}")
    return 1 if res is None else 0


if __name__ == "__main__":
    sys.exit(main())
