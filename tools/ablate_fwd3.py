"""Times the split-bf16 forward of every variant built by tools/ablate_fwd3.sh (one child process per library)."""
import glob, os, sys

import ab_harness

CHILD = r'''
import torch, bench, lsnf_amd
dev = torch.device("cuda:0")
plan = lsnf_amd.prepare([t.to(dev) for t in bench.synth_weights(1)], bench.NZ, bench.WIDTH, bench.DEPTH)
z = torch.randn(65536, bench.NZ, generator=torch.Generator().manual_seed(1234)).to(dev)
lsnf_amd.flow.set_math_mode(1)
out = (torch.empty_like(z), torch.empty(65536, device=dev), torch.empty(65536, device=dev))
for _ in range(800): lsnf_amd.forward(plan, z, out=out)
torch.cuda.synchronize()
emit("%7.1f us" % windows(lambda: lsnf_amd.forward(plan, z, out=out), 300, 1)[0])
'''


def main(argv=None):
    libs = sorted(glob.glob(os.path.join(ab_harness.ROOT, "latent-space-normalizing-flow_amd", "_ablate", "f3_*.so")))
    res = ab_harness.run(CHILD, [(os.path.basename(lib), lib, {}) for lib in libs], timeout=120, ok=lambda tag, r, t: f"{tag:28s} {t}")
    return 1 if res is None else 0


if __name__ == "__main__":
    sys.exit(main())
