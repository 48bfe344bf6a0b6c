"""GPU A/B: f_width 128 throughput forward as shipped (hipcc spills ~48 registers to scratch in the 8-wave instantiation)
against a -DLSNF_PARK_V build that parks v1 / v2 in the wave's own z_out rows instead (zero scratch), alternating in one
job.  Variant: hipcc ... -DLSNF_PARK_V -c lsnf_fwd3.hip / lsnf_fwd2h.hip, linked with the other objects into
latent-space-normalizing-flow_amd/_ablate/park.so.  Result (profiles/r02_ab_c5_park.txt): parked 186 us vs 153 us."""
import os, sys

import ab_harness

CHILD = r'''
import os, sys, types, numpy as np, torch
import lsnf_amd
dev = torch.device("cuda:0")
def timeit(fn, n=300, warm=600):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    return windows(fn, n, 1)[0]
hps = types.SimpleNamespace(f_n_levels=1, f_depth=5, f_flow_permutation=2, f_width=128, f_flow_coupling=1)
torch.manual_seed(1); np.random.seed(1)
net = lsnf_amd._netF(hps, nz=100).to(dev); plan = net._plan()
z = torch.randn(65536, 100, device=dev)
out = (torch.empty_like(z), torch.empty(65536, device=dev), torch.empty(65536, device=dev))
r = []
for mode, nm in ((1, "bf16x3"), (3, "fp16x2")):
    lsnf_amd.flow.set_math_mode(mode)
    r.append("%s %.1f us" % (nm, timeit(lambda: lsnf_amd.forward(plan, z, out=out))))
emit("  ".join(r))
'''


def main(argv=None):
    park = os.path.join(ab_harness.ROOT, "latent-space-normalizing-flow_amd", "_ablate", "park.so")
    res = ab_harness.run(CHILD, [("hipcc spills (shipped)", None, {}), ("parked (-DLSNF_PARK_V)", park, {})], rounds=2, timeout=200,
                         ok=lambda name, r, line: f"C5 nz=100 w=128 B=65536 forward, {name:24s}: {line}")
    return 1 if res is None else 0


if __name__ == "__main__":
    sys.exit(main())
