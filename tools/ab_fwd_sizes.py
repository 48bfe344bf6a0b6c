"""GPU A/B of two builds of the library on the plain forward (+ in-kernel sums) at the strong-scaling shard sizes and the full size:
python tools/ab_fwd_sizes.py LIB_A LIB_B  (each size timed alternately, three rounds; a child process per library and round;
"LIB round R: ok" after each child, then the table)."""
import sys

import ab_harness

CHILD = r'''
import os, sys, torch
import bench, lsnf_amd
F = lsnf_amd.flow
dev = torch.device("cuda:0")
plan = lsnf_amd.prepare([t.to(dev) for t in bench.synth_weights(1)], bench.NZ, bench.WIDTH, bench.DEPTH)
res = {}
for B in (65536, 32768, 16384, 8192):
    z = torch.randn(B, bench.NZ, device=dev)
    outs = (torch.empty_like(z), torch.empty(B, device=dev), torch.empty(B, device=dev))
    st = F.new_stats(dev)
    for _ in range(600): lsnf_amd.forward(plan, z, out=outs, stats=st)
    torch.cuda.synchronize()
    res[B] = sorted(windows(lambda: lsnf_amd.forward(plan, z, out=outs, stats=st), 300, 5))[2]
emit(res)
'''


def main(argv=None):
    libs = (sys.argv[1:] if argv is None else argv)[:2]
    acc = ab_harness.run(CHILD, [(l, l, {}) for l in libs], rounds=3, timeout=280)
    if acc is None:
        return 1
    for l in libs:
        print(l)
        for B in ("65536", "32768", "16384", "8192"):
            v = sorted(r[B] for r in acc[l])
            print(f"   B={B:>6}: median {v[1]:7.2f} us  (min {v[0]:.2f}, max {v[2]:.2f})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
