"""GPU: time the ablation builds of tools/ablate_fwd3p.sh (one subprocess per build, B = 65 536, kernel-only loop)."""
import glob, os, sys

import ab_harness

CHILD = r'''
import os, sys, torch
import bench, lsnf_amd
dev = torch.device("cuda:0")
plan = lsnf_amd.prepare([t.to(dev) for t in bench.synth_weights(1)], bench.NZ, bench.WIDTH, bench.DEPTH)
lsnf_amd.flow.set_math_mode(lsnf_amd.flow.MATH_BF16X3)
z = torch.randn(65536, bench.NZ, generator=torch.Generator().manual_seed(1234)).to(dev)
outs = (torch.empty_like(z), torch.empty(65536, device=dev), torch.empty(65536, device=dev))
for _ in range(1500): lsnf_amd.forward(plan, z, out=outs)
torch.cuda.synchronize()
emit("%8.2f us" % windows(lambda: lsnf_amd.forward(plan, z, out=outs), 500, 1)[0])
'''


def main(argv=None):
    libs = sorted(glob.glob(os.path.join(ab_harness.ROOT, "latent-space-normalizing-flow_amd", "_ablate", "p_*.so")))
    res = ab_harness.run(CHILD, [(os.path.basename(so), so, {}) for so in libs], timeout=120, ok=lambda tag, r, t: f"{tag:40s} {t}")
    return 1 if res is None else 0


if __name__ == "__main__":
    sys.exit(main())
