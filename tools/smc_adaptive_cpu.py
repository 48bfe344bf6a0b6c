"""The adaptive-tempering SMC experiment of tests/hmc_schedule_restated.py on the CPU (float64, no GPU): writes what
profiles/smc_adaptive_cpu.txt holds and prints the bands of hmc_schedule_restated.BAND.

    python tools/smc_adaptive_cpu.py > profiles/smc_adaptive_cpu.txt

Seeds 0 .. 7, both spaces, max_steps = 40, CESS targets 0.90 / 0.95 / 0.98; the bands are made for the target the tests use
(hmc_schedule_restated.EXP_TARGET) exactly as profiles/smc_cpu.txt's: [smallest - 3 SD, largest + 3 SD]."""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ais_restated as A  # noqa: E402
import hmc_schedule_restated as S  # noqa: E402
import smc_restated as SM  # noqa: E402

SEEDS = range(8)
TARGETS = (0.90, 0.95, 0.98)


def sd(v):
    return torch.tensor(v, dtype=torch.float64).std(unbiased=True).item()


def band(v, s, digits):
    return round(min(v) - 3.0 * s, digits), round(max(v) + 3.0 * s, digits)


def main():
    K = S.EXP_MAX_STEPS
    print("# The adaptive-tempering experiment of tests/hmc_schedule_restated.py (experiment), float64 restatement on the CPU, no GPU involved:")
    print("# the problem, the closed forms, the 2 data x 64 chains = 128 rows, L = 3, the frozen step 0.28 and the unit metric are")
    print(f"# profiles/ais_cpu.txt's; groups of 16 particles, ess_threshold 0.5, max_steps = {K}, min_step = 1 / (4 max_steps), and the draws of")
    print("# tests/smc_restated.py (the same generator).  The init call and the end calls k < max_steps - 1 search the next temperature")
    print("# (twelve halvings on the CESS of the group's incremental weights), end call max_steps - 1 goes to 1 in one plain step.")
    print("# Figures of a run: per datum the error log Z_hat - closed form and the effective sample size of its 64 final weights; the mean")
    print("# acceptance of its max_steps x 128 decisions; the annealing calls each of the 8 groups entered below beta = 1 (steps used).")
    print("# The bands: [smallest - 3 SD, largest + 3 SD] over the 16 estimates (error, ess), the 64 groups (steps); acceptance: SE =")
    print("# sqrt(p (1 - p) / decisions) at the observed mean, as profiles/smc_cpu.txt's.")
    bands, finding = {}, []
    for space in ("z", "eps"):
        for target in TARGETS:
            print(f"# ---- {space}, adaptive SMC, CESS target {target}, 16 particles ----")
            errs, esss, accs, used = [], [], [], []
            for seed in SEEDS:
                e, s, a, u = S.experiment(seed, space, cess_target=target)
                errs += e.tolist(); esss += s.tolist(); accs.append(a); used += u.tolist()
                print(f"seed {seed}: errors {e[0]:+.4f} {e[1]:+.4f}; ess {s[0]:.2f} {s[1]:.2f}; mean acceptance {a:.4f}; steps used "
                      + " ".join(str(int(v)) for v in u.tolist()) + f" of {K}")
            se, ss, su = sd(errs), sd(esss), sd(used)
            p = sum(accs) / len(accs)
            sa = math.sqrt(p * (1.0 - p) / (K * 128))
            b = {"error": band(errs, se, 3), "ess": band(esss, ss, 1), "accept": band(accs, sa, 3), "steps": band(used, su, 1)}
            inside = "lies inside" if b["error"][0] < 0.0 < b["error"][1] else "LIES OUTSIDE"
            print(f"error: estimates {min(errs):+.4f} .. {max(errs):+.4f}, mean {sum(errs) / len(errs):+.4f}, standard deviation over the 16 estimates "
                  f"{se:.4f} -> {b['error']}; the closed form (0) {inside}")
            print(f"ess: estimates {min(esss):.2f} .. {max(esss):.2f} of 64, standard deviation over the 16 estimates {ss:.2f} -> {b['ess']}")
            print(f"acceptance: runs {min(accs):.4f} .. {max(accs):.4f}, mean {p:.4f}, SE({K * 128} decisions) = {sa:.4f} -> {b['accept']}")
            print(f"steps used: groups {int(min(used))} .. {int(max(used))}, mean {sum(used) / len(used):.1f}, standard deviation over the 64 groups "
                  f"{su:.2f} -> {b['steps']}")
            bands[(space, target)] = b
            finding.append((space, f"adaptive {target}", sum(used) / len(used), se, sum(errs) / len(errs), sum(esss) / len(esss)))
        for T in (SM.SHORT_T, A.EXP_T):
            errs, esss = [], []
            for seed in SEEDS:
                e, s, _, _ = SM.experiment(seed, space, T=T)
                errs += e.tolist(); esss += s.tolist()
            finding.append((space, f"fixed T = {T}", float(T), sd(errs), sum(errs) / len(errs), sum(esss) / len(esss)))
    print("# ---- the finding (fixed: tests/smc_restated.py experiment, the sigmoid schedule, the same seeds) ----")
    for space, kind, steps, se, me, es in finding:
        print(f"# {space}, {kind}: annealing steps {steps:.1f}; standard deviation of log Z_hat over the 16 estimates {se:.4f}; mean error {me:+.4f}; "
              f"mean final ess of 64: {es:.1f}")
    print("# ---- hmc_schedule_restated.BAND ----")
    for space in ("z", "eps"):
        print(f"# \"{space}\": {bands[(space, S.EXP_TARGET)]}")


if __name__ == "__main__":
    main()
