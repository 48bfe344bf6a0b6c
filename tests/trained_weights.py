"""The chain tests' cases at weights of trained size: one table for tests/test_gpu_mala.py, test_gpu_rmala.py, test_gpu_hmc.py,
test_gpu_rhmc.py, test_gpu_reverse_keep.py, test_gpu_reverse_langevin.py and the HMC levels that stand on them (not a test module;
tests/test_trained_weights_cpu.py holds the table to what it claims).

Every other chain case builds its flow with oracle.init_params(seed=3): weights of scale 0.05, the coupling's sigmoid(h + 2) near 0.88,
exp(3 logs) near 1, |grad log p| of order 10.  The cases here take the weights of the trained golden fixtures instead -- a saturating
sigmoid, |3 logs| up to 2, gradients of order 1e3 -- and nothing else of them: the batch stays each Case's own oracle.smooth_batch.  A
`Case(..., weights="trained")` of those modules is built on them; the default, "init", is what it was.

At these weights the float64 leapfrog is stable only in a narrow window of step sizes (C3 in z: 98 % accepted at 0.04, 3 % at 0.06,
ll = -inf at 0.2), so the step tables of the test modules do not carry over.  STEP holds one step per case class and geometry, chosen
the way those tables are: on the CPU, from `Case.rate` of the 33-row case alone (the float64 restatement), scanned in steps of 0.005
(C3, C5) and 0.05 (TINY); the step whose rate is nearest one half, the smaller of two.  The rate found is beside each entry; the whole
scan is in profiles/chain_trained.txt.  No step, seed or row set is chosen from a device's answer."""
from conftest import load_golden

C3, C5, TINY = (128, 64, 5, 1), (100, 128, 5, 1), (8, 4, 5, 1)
INIT, TRAINED = "init", "trained"

# geometry -> the golden fixture whose sd/ tensors are the weights: one per <HT, WT> instantiation (<2, 2>, <2, 4>, <1, 1>)
WEIGHTS = {C3: "c3_nz128_w64_B65_trained02", C5: "c5_nz100_w128_B33_trained02", TINY: "tiny_nz8_w4_B37_trained"}

# C3 at 16, 32 and 64 rows per workgroup (4100 and 8200 end ragged); C5, <2, 4>, at both of its shapes; TINY
CASES = [C3 + (33,), C3 + (100,), C3 + (4100,), C3 + (8200,), C5 + (33,), C5 + (4100,), TINY + (33,)]
SMALL = [C3 + (33,), C5 + (33,), TINY + (33,)]
# the exchange, resampling and schedule checks, (geometry, B, R or P): 24 rows of R = P = 8 (a ragged tile) and 32 rows of 16
LADDERS = [g + bR for g in (C3, TINY) for bR in ((24, 8), (32, 16))]

# case class -> geometry -> step.  Beside each entry: the float64 rate of the 33-row case (two trajectories of L = 3, or three MALA steps)
STEP = {
    "hmc z": {C3: 0.05, C5: 0.09, TINY: 0.6},            # 0.64 / 0.30 / 0.48
    "hmc eps": {C3: 0.025, C5: 0.03, TINY: 0.45},        # 0.62 / 0.47 / 0.29
    "mala z": {C3: 0.06, C5: 0.095, TINY: 0.6},          # 0.29 / 0.49 / 0.56
    "mala eps": {C3: 0.03, C5: 0.035, TINY: 0.45},       # 0.35 / 0.40 / 0.48
}
# The reverse-Langevin step (tests/test_gpu_reverse_langevin.py): no decision, so no rate.  The float64 update eps - s^2 / 2 (eps + g)
# + s xi of the 33-row case (tests/test_gpu_reverse_keep.py's inputs, that module's noise) scanned over s = 0.01, 0.02, 0.03, 0.05, 0.1,
# 0.2, 0.3, 0.5, 1: the largest step at which x = f^-1(eps_next) stays finite and within 10 on every row.  Found: max |x| = 9.7 / 8.1 /
# 6.6 (one step on: 28 / 31 / 14; at 0.5 x is inf on C3 and NaN on C5).
LANGEVIN_STEP = {C3: 0.05, C5: 0.05, TINY: 0.2}

# A diverging trajectory (tests/test_gpu_hmc.py, test_gpu_rhmc.py: C3, 33 rows): the step at which the float64 records hold ll = -inf
# and a NaN gradient from the second inner call on.  z: measured at 0.2 (18 of 33 rows NaN there, every log_alpha NaN).  eps: the
# smallest multiple of 0.05 that shows the same (25 rows; at 0.05 all 33 log_alpha are NaN or below -100 already, but the gradient is
# NaN on 8 rows of the end call alone).
DIVERGING_STEP = {"hmc z": 0.2, "hmc eps": 0.1}
DIVERGING_ROWS = 30                          # float64 log_alpha is NaN, -inf or below -100 on at least so many of the 33 rows
# At both steps all 33 rows diverge, which would leave "no other row differs from the call on those rows alone" nothing to run on.  So
# three rows, one in each 16-row tile, are given the end call's inputs of the same case at its stable step (STEP) instead: rows with
# finite inputs beside 30 diverged ones, in one launch at the diverging step.
GRAFTED = (0, 16, 32)


def params_of(geo):
    """The trained weights of a geometry: the fixture's state dict, as tests/test_gpu_module.py loads it."""
    params, rest = load_golden(WEIGHTS[geo])
    assert (int(rest["meta_nz"]), int(rest["meta_width"]), int(rest["meta_depth"])) == geo[:3]
    return params


def params_for(O, geo, weights):
    """A Case's flow: oracle.init_params(seed=3) for "init", the golden trained weights for "trained"."""
    if weights == INIT:
        return O.init_params(*geo[:3], seed=3)
    assert weights == TRAINED and geo in WEIGHTS, (geo, weights)
    return params_of(geo)


def graft(record, stable, rows=GRAFTED):
    """A copy of a call record in which every per-row tensor holds `stable`'s rows at `rows`."""
    import copy
    import torch
    out, idx = copy.copy(record), list(rows)
    for k, v in vars(record).items():
        w = getattr(stable, k, None)
        if torch.is_tensor(v) and torch.is_tensor(w) and v.shape == w.shape and v.dim() >= 1 and v.shape[0] > max(idx):
            v = v.clone()
            v[idx] = w[idx]
            setattr(out, k, v)
    return out


def step_of(kind, geo):
    return STEP[kind][geo]
