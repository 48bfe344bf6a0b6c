"""GPU: every value of the workgroup-shape knobs of INTEGRATION.md section 4 -- LSNF_FWD3Q_SHAPE, LSNF_SMALL3_ST, LSNF_FORCE_WAVES,
LSNF_FWD_WAVES, LSNF_TN_PLAIN, LSNF_TN_X3, LSNF_TN_CHUNK -- at the batch sizes where a workgroup shape goes wrong: B = 1, 17, one short
of / equal to / one past a workgroup of R rows, and a ragged third workgroup (2R + 33), R computed from the knob value
(tests/shape_forms_worker.py holds the table); nothing larger except the sizes at which the code itself changes path (4 096: the
LDS-staged batch contraction; 12 288: the tiled parameter-gradient dump and the bf16 contraction).

The knobs are read once per process, so each setting runs in a fresh child (tests/shape_forms_worker.py, the pattern of
tests/test_gpu_fwd3q_pair.py), one after another, each under its own `timeout`; after the first child that exits non-zero no further
child is started and every test of the module fails with that child's output.  The float64 oracle is evaluated here, once per
geometry: a case of B rows is the first B rows of the geometry's master batch.

Gates are the project's existing ones, each cited where it is defined below; none is new.  Bit identity is asserted where the project
claims it, every run against the longest run of its key on all the rows it has (hold_to_longest), so the rows around each workgroup
edge are compared: z1 and the block outputs across every bf16x3 forward ("rows do not depend on the batch size");
z1 / logdet / ll between LSNF_FWD3Q_SHAPE 242, 82 and 42 (32 rows per wave, tests/test_gpu_fwd3q_pair.py); the in-kernel draws across
every form (tests/test_gpu_sample.py); everything across LSNF_SMALL3_ST for the two MALA kernels (test 4 of tests/test_gpu_mala.py /
test_gpu_rmala.py) -- at equal batch sizes only, since a MALA case is seeded by its size: 1, 17 and 97 in every child.  Limits: the
stash words are compared for whole 32-row tiles at equal B only (the rows of a ragged tile past the batch are not defined), across
kernel families on C3 and within a family elsewhere (padded feature columns).
4 against 8 waves: lsnf_fwd3b_kernel, lsnf_rev3_kernel and lsnf_bwd3_kernel were read -- the wave count enters a wave's first row, the
weight staging, the constants' copy, the fix-up flag and the order of the batch sums only -- and their per-row outputs are held to bits
(test_four_and_eight_wave_forms_give_the_same_rows) except the forward's per-row ll, which the two code objects of the <1, 1> geometry
round differently on a few rows (that test's docstring has the figures); lsnf_fwd_kernel and the fp16x2 pair (whose fix-up recomputes
whole workgroups, so a row may come from either arithmetic depending on the workgroup's extent) are held to the float64 gates alone.

Wall time of a child on one MI355X: 3.0 to 7.7 s (process start-up, the import of torch and the library's load dominate; the six
children together 37 s of the module's 52 s); limit of each child 60 s, more than 7 x the slowest (TIMEOUT below has both numbers)."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from oracle import flow_oracle as O
import reverse_restated as R
import sample_restated as S
import shape_forms_worker as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL_REL_F64 = 2e-6      # tests/test_gpu_forward.py::test_split_bf16_is_fp32_faithful: the bf16x3 forward's log-prob against float64
LL_REL = 1e-5          # tests/test_gpu_forward.py: log-prob, relative per row, every other arithmetic
Z_ABS = 1e-4           # tests/test_gpu_forward.py: z1 against the oracle, of max(1, max|z1|)
REV_X = 5e-5           # tests/test_gpu_reverse_backward.py inverse_tolerance's floor: the reverse, of max(1, max|x|)
OBJ_REL = 1e-5         # tests/test_gpu_reverse_backward.py::test_reverse_matches_reference_golden: objective_out
GZ_REL = 1e-5          # tests/test_gpu_param_grads_oracle.py TOL_GZ / tests/test_gpu_reverse_backward.py: dz, relative L2
LV_ABS = 2e-5          # tests/test_gpu_langevin.py: z_new of one Langevin step
NORM_REL = 1e-5        # tests/test_gpu_langevin.py: gf_norm / gg_norm
RBWD_FLOOR = 1e-5      # tests/test_gpu_reverse_autograd.py: max(1e-5, 3 x the oracle's own fp32-vs-fp64 error on that input)
PARAM_REL = 2e-5       # tests/test_gpu_param_grads_oracle.py TOL: parameter gradients, relative L2 per tensor
SUMS_REL = 1e-9        # tests/test_gpu_fwd3q_pair.py: the in-kernel sums against the arrays the same call wrote
# child -> (measured wall seconds on one MI355X, limit = at least 3 x that)
TIMEOUT = {"baseline": (6.9, 60), "q41_w4_st1_chunk16": (7.7, 60), "q81_w8_st2_chunk4096": (7.7, 60), "q42_st4_plain": (7.5, 60),
           "q82_x3off": (3.0, 60), "q242_chunk24": (4.2, 60)}
NAMES = [name for name, _ in W.CHILDREN]
BF16X3 = ("q.", "w.phased.", "w.bwd", "s.")          # probes whose forward runs the bf16x3 arithmetic


@pytest.fixture(scope="module")
def forms(gpu_device, tmp_path_factory):
    """({child: arrays}, None), or ({}, the output of the first child that ended non-zero): children run one after another and none is
    started after a failure."""
    d = tmp_path_factory.mktemp("shape_forms")
    got = {}
    worker = os.path.join(ROOT, "tests", "shape_forms_worker.py")
    for name, env in W.CHILDREN:
        out = str(d / f"{name}.npz")
        child_env = {k: v for k, v in os.environ.items() if k not in W.KNOB_VALUES}
        child_env.update(env)
        t0 = time.time()
        r = subprocess.run(["timeout", "-k", "10", str(TIMEOUT[name][1]), sys.executable, worker, name, out], env=child_env,
                           capture_output=True, text=True)
        say(f"child {name} {env}: exit {r.returncode}, {time.time() - t0:.1f} s (limit {TIMEOUT[name][1]} s)")
        if "small3" in W.groups_of(env):         # which ST each geometry's latency kernels really ran (lsnf_small3_*_st's rules, as the worker's table has them)
            say(f"child {name}: LSNF_SMALL3_ST wanted {W.small3_st(env, 'C3')[0]}, ran " + ", ".join(f"{g} ST {W.small3_st(env, g)[1]}" for g in W.GEOS))
        if r.returncode != 0:
            return {}, f"child {name} {env} ended with {r.returncode}; its last lines:\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
        got[name] = dict(np.load(out))
    return got, None


@pytest.fixture
def got(forms):
    arrays, failure = forms
    if failure:
        pytest.fail(failure)
    return arrays


# ---- the float64 oracle, once per geometry ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle(geo, n=W.N_SMALL):
    p, m = W.master(geo, n)
    p64 = O.to_dtype(p, torch.float64)
    z = m["z"].double().requires_grad_(True)
    z1, ld = O.flow_forward(p64, z, torch.zeros(n, dtype=torch.float64))
    ll = O.log_prob(z1, ld)
    (gz,) = torch.autograd.grad(-ll.sum(), z)
    o = {"z1": z1.detach(), "logdet": ld.detach(), "ll": ll.detach(), "gz": gz, "obj": m["obj"].double()}
    if n == W.N_SMALL:
        x, negobj = O.flow_reverse(p64, m["eps"].double(), m["obj"].double())
        o["x"], o["objout"] = x, -negobj
        zero = torch.zeros(n)
        o["geps"] = R.reverse_loss_grads(p, m["eps"], zero, m["gx"], m["go"], torch.float64)[2]
        o["geps32"] = R.reverse_loss_grads(p, m["eps"], zero, m["gx"], m["go"], torch.float32)[2]
        o["gf_norm"] = gz.norm(dim=1)
    return o


@functools.lru_cache(maxsize=64)
def param_ref(geo, n, B):
    """d(-mean ll)/dtheta over the first B rows of the master batch, float64, as the flat buffer of flow.backward_params lays it out."""
    import lsnf_amd
    p, m = W.master(geo, n)
    p64 = O.to_dtype(p, torch.float64)
    keys = [O.block_prefix(i) + k for i in range(W.GEOS[geo][2]) for k in lsnf_amd.flow.BLOCK_PARAM_KEYS]
    live = {k: p64[k].clone().requires_grad_(True) for k in keys}
    _, _, ll = O.flow_log_prob({**p64, **live}, m["z"][:B].double(), W.GEOS[geo][3])
    grads = torch.autograd.grad(-ll.mean(), [live[k] for k in keys])
    return keys, [g.reshape(-1) for g in grads]


def say(line):
    """A record line of profiles/shape_forms.txt (pytest -s): on a line of its own, whatever the progress output before it."""
    print("\n[shape-forms] " + line)


class Worst:
    """Worst measured error / gate per (child, probe), printed for profiles/shape_forms.txt (pytest -s)."""

    def __init__(self, child):
        self.child, self.rows, self.bad = child, {}, []

    def add(self, probe, what, err, gate, where):
        k = (probe, what)
        if k not in self.rows or err / gate > self.rows[k][0] / self.rows[k][1]:
            self.rows[k] = (err, gate, where)
        if not err <= gate:
            self.bad.append((probe, what, where, err, gate))

    def done(self):
        for (probe, what), (err, gate, where) in sorted(self.rows.items()):
            say(f"{self.child:<22} {probe:<16} {what:<12} worst {err:.3e}  gate {gate:.3e}  at {where}")
        assert not self.bad, self.bad[:10]


def split(arrays):
    """{(probe, geo, B): {array name: array}} of one child."""
    out = {}
    for k, a in arrays.items():
        probe, geo, B, name = k.split("|")
        out.setdefault((probe, geo, int(B[1:])), {})[name] = a
    return out


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def rows_of(geo, B):
    return W.N_LARGE if B > W.N_SMALL else W.N_SMALL


# ---- against float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("child", NAMES)
def test_forward_outputs_meet_float64(got, child):
    """z1 and the log-prob of every forward probe (plain, stats, each stash combination, the dump-writing forward, the forwards inside
    the backward and parameter-gradient probes) against float64; no NaN left in an output that was NaN-filled, the sentinel behind the
    outputs untouched, the in-kernel sums those of the arrays the same call wrote and the row count exact."""
    w, n_checked = Worst(child), 0
    for (probe, geo, B), a in sorted(split(got[child]).items()):
        if "guard" in a:
            assert a["guard"].tolist() == [7.0, 7.0], (probe, geo, B, a["guard"])
        for name, arr in a.items():
            if not name.startswith(("act", "guard")):
                assert np.isfinite(arr).all(), (probe, geo, B, name)
        if "ll" not in a or "eps" in a or probe in ("s.mala", "s.rmala"):      # (`sample`'s ll_out and the MALA calls: their own tests below)
            continue
        o = oracle(geo, rows_of(geo, B))
        obj = o["obj"][:B].numpy() if "sums" in a else 0.0
        z1r, llr = o["z1"][:B].numpy(), o["ll"][:B].numpy() + obj
        if "z1" in a:
            w.add(probe, "z1", float(np.abs(a["z1"] - z1r).max()), Z_ABS * max(1.0, float(np.abs(z1r).max())), f"{geo} B{B}")
        w.add(probe, "ll", float((np.abs(a["ll"] - llr) / np.maximum(np.abs(llr), 1.0)).max()),
              LL_REL_F64 if probe.startswith(BF16X3) else LL_REL, f"{geo} B{B}")
        if "logdet" in a and "sums" in a:
            s, ll, ld = a["sums"], a["ll"].astype(np.float64).sum(), a["logdet"].astype(np.float64).sum()
            assert s[2] == B, (probe, geo, B, s)
            w.add(probe, "sum ll", abs(s[0] - ll), SUMS_REL * abs(ll) + 1e-9, f"{geo} B{B}")
            w.add(probe, "sum logdet", abs(s[1] - ld), SUMS_REL * abs(ld) + 1e-9, f"{geo} B{B}")
        n_checked += 1
    w.done()
    assert n_checked > 0


@pytest.mark.parametrize("child", NAMES)
def test_reverse_and_sample_meet_float64(got, child):
    """x and objective_out of the reverse (plain and stash-keeping) against float64; the fused sample against the float64 flow at its
    own draws, its ll_out against its own outputs (tests/test_gpu_sample.py _check_flow)."""
    w = Worst(child)
    for (probe, geo, B), a in sorted(split(got[child]).items()):
        if "x" not in a:
            continue
        if "eps" in a:
            x64, _, _ = S.flow_at(W.params_of(geo), torch.from_numpy(a["eps"]))
            own = S.ll(torch.from_numpy(a["eps"]).double(), torch.from_numpy(a["objout"]).double()).numpy()
            w.add(probe, "ll_out", float((np.abs(a["ll"] - own) / np.maximum(np.abs(own), 1.0)).max()), LL_REL, f"{geo} B{B}")
            xr = x64.numpy()
        else:
            if B == W.BIG:
                eps, obj = W.big_inputs(geo)
                x64, negobj = O.flow_reverse(O.to_dtype(W.params_of(geo), torch.float64), eps.double(), obj.double())
                xr, objr = x64.numpy(), -negobj.numpy()
            else:
                o = oracle(geo)
                xr, objr = o["x"][:B].numpy(), o["objout"][:B].numpy()
            w.add(probe, "objective", float((np.abs(a["objout"] - objr) / np.maximum(np.abs(objr), 1.0)).max()), OBJ_REL, f"{geo} B{B}")
        w.add(probe, "x", float(np.abs(a["x"] - xr).max()), REV_X * max(1.0, float(np.abs(xr).max())), f"{geo} B{B}")
    w.done()


@pytest.mark.parametrize("child", NAMES)
def test_gradients_meet_float64(got, child):
    """dz from the stash, the Langevin step with tensor and with in-kernel noise (the draw is `sample`'s eps of the same generator),
    the reverse-backward and the base-space Langevin step (its g is reverse_backward_z's bit for bit, its update within the rounding
    bound of tests/test_gpu_reverse_langevin.py::test_update_arithmetic).  Kink-free rows: none is set aside."""
    w, cases = Worst(child), split(got[child])
    for (probe, geo, B), a in sorted(cases.items()):
        where = f"{geo} B{B}"
        if probe in ("w.bwd", "s.bwd"):
            w.add(probe, "dz", rel_l2(a["gz"], oracle(geo)["gz"][:B].numpy()), GZ_REL, where)
        elif probe.endswith(".lv.tensor") or probe.endswith(".lv.philox"):
            o, m = oracle(geo), W.master(geo)[1]
            noise = m["noise"][:B].double().numpy() if probe.endswith("tensor") else \
                cases[(probe.split(".")[0] + ".sample", geo, B)]["eps"].astype(np.float64)
            gg = m["gg"][:B].double().numpy()
            ref = m["z"][:B].double().numpy() - 0.5 * W.STEP ** 2 * (gg + o["gz"][:B].numpy()) + W.STEP * noise
            w.add(probe, "z_new", float(np.abs(a["z_new"] - ref).max()), LV_ABS, where)
            gfr, ggr = o["gf_norm"][:B].numpy(), np.linalg.norm(gg, axis=1)
            w.add(probe, "gf_norm", float((np.abs(a["gf"] - gfr) / gfr).max()), NORM_REL, where)
            w.add(probe, "gg_norm", float((np.abs(a["ggn"] - ggr) / ggr).max()), NORM_REL, where)
        elif probe == "s.rbwd":
            o = oracle(geo)
            ref, own = o["geps"][:B].numpy(), rel_l2(o["geps32"][:B].numpy(), o["geps"][:B].numpy())
            w.add(probe, "d eps", rel_l2(a["geps"], ref), max(RBWD_FLOOR, 3.0 * own), where)
            lv = cases[("s.rbwd.lv", geo, B)]
            assert np.array_equal(lv["g"].view(np.uint32), a["geps_x"].view(np.uint32)), where     # tests/test_gpu_reverse_langevin.py::test_gradient_bits
            m = W.master(geo)[1]
            e, n, g, coef = m["eps"][:B].double().numpy(), m["noise"][:B].double().numpy(), lv["g"].astype(np.float64), 0.5 * W.STEP ** 2
            r = e - coef * (e + g) + W.STEP * n
            bound = 2.0 ** -23 * (np.abs(e) + 3.0 * coef * np.abs(e + g) + 2.0 * W.STEP * np.abs(n))
            w.add("s.rbwd.lv", "update", float((np.abs(lv["eps_new"] - r) / bound).max()), 1.0, where)
    w.done()


@pytest.mark.parametrize("child", NAMES)
def test_parameter_gradients_meet_float64(got, child):
    """Every tensor of the fast path and of the recomputing path, and dL/dz, against float64 on `oracle.smooth_batch` rows."""
    w = Worst(child)
    for (probe, geo, B), a in sorted(split(got[child]).items()):
        if "flat" not in a:
            continue
        n = rows_of(geo, B)
        keys, refs = param_ref(geo, n, B)
        off = 0
        for k, r in zip(keys, refs):
            w.add(probe, "d theta", rel_l2(a["flat"][off:off + r.numel()], r.numpy()), PARAM_REL, f"{geo} B{B} {k}")
            off += r.numel()
        assert off == a["flat"].size
        if "gz" in a:
            w.add(probe, "dz", rel_l2(a["gz"], oracle(geo, n)["gz"][:B].numpy() / B), GZ_REL, f"{geo} B{B}")
    w.done()


def _t(a):
    return torch.from_numpy(a)


@pytest.mark.parametrize("child", NAMES)
def test_mala_steps_follow_float64(got, child):
    """The teacher-forced first step of tests/test_gpu_mala.py / tests/test_gpu_rmala.py (their Case and run) under the forced shape:
    their per-row gate and set-aside cap, unchanged."""
    import test_gpu_mala as ZM
    import test_gpu_rmala as RMt
    n = 0
    for (probe, geo, B), a in sorted(split(got[child]).items()):
        if probe not in ("s.mala", "s.rmala"):
            continue
        n += 1
        T = ZM if probe == "s.mala" else RMt
        c = T.case(*W.geo_of(geo), B)
        st = c.steps[0]
        la, acc = _t(a["la"]).double(), _t(a["acc"])
        za, ga, ua, nxt = _t(a["state_z"]), _t(a["state_grad"]), _t(a["state_energy"]), _t(a["z_next"])
        aside, allowed = int((~st.decided).sum()), (2 if B <= 33 else B // 10)
        err = (la - st.la).abs()
        worst = (err / st.gate)[st.smooth].max().item() if bool(st.smooth.any()) else 0.0
        say(f"{child:<22} {probe:<16} {geo} B{B}: set aside {aside} (allowed {allowed}), worst |log_alpha - fp64| / gate {worst:.3f}")
        assert aside <= allowed
        assert bool((err <= st.gate)[st.smooth].all())
        d, a64 = st.decided, st.acc
        assert bool(((acc == 1.0) | (acc == 0.0)).all()) and torch.equal(acc[d] == 1.0, a64[d])
        yes, no = d & a64, d & ~a64
        f32 = lambda t: t.float()
        if probe == "s.mala":
            assert ZM.bits(za[yes], f32(st.z_prop)[yes])
            assert bool(((ua[yes].double() - st.U_prop[yes]).abs() <= 1e-5 * (st.e[yes].abs() + st.ll[yes].abs())).all())
            assert bool((ZM.rel_rows(ga[yes], st.g_prop[yes]) <= 1e-5).all())
            assert ZM.bits(za[no], f32(st.z_acc)[no]) and ZM.bits(ga[no], f32(st.g_acc)[no]) and ZM.bits(ua[no], f32(st.u_acc)[no])
            assert bool((ZM.rel_rows(nxt[d], st.z_next[d]) <= 1e-5).all())
        else:
            assert ZM.bits(za[yes], f32(st.e_prop)[yes])
            assert ZM.bits(za[no], f32(st.e_acc)[no]) and ZM.bits(ga[no], f32(st.t_acc)[no]) and ZM.bits(ua[no], f32(st.u_acc)[no])
            if bool(yes.any()):
                u_bound = torch.maximum(1e-5 * st.u_scale, 3.0 * st.u_own)[yes]
                assert bool(((ua[yes].double() - st.U_prop[yes]).abs() <= u_bound).all())
                assert RMt.rel_l2(ga[yes], st.t_prop[yes]) <= max(1e-5, 3.0 * RMt.rel_l2(st.t32[yes], st.t_prop[yes]))
            n_err = RMt.rel_l2(nxt[d], st.e_next[d]) if bool(d.any()) else 0.0
            assert n_err <= max(1e-5, 3.0 * RMt.rel_l2(st.t32, st.t_prop))
    assert n > 0 or "small3" not in W.groups_of(dict(W.CHILDREN)[child])


# ---- bit identity across forms -----------------------------------------------------------------------------------------------
def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def whole_tiles(act, geo, B):
    """The words of the complete 32-row tiles of an activation stash (csrc/lsnf_layout.h lsnf_act_layout: per block ceil(B / 32) tiles)."""
    depth, tiles = W.GEOS[geo][2], (B + 31) // 32
    per_tile = act.size // (depth * tiles)
    return act[: depth * tiles * per_tile].reshape(depth, tiles, per_tile)[:, : B // 32]


def hold_to_longest(runs, names, more_than):
    """runs: [(label, B, arrays)] of one key.  The longest run is the reference; the arrays `names` of EVERY run are the first B rows
    of the reference's, bit for bit (so any two runs agree on the rows they share), and the longest comparison against another run
    covers more than `more_than` rows -- more than a workgroup, so the rows around its edge are among those compared.  Returns the
    number of runs compared."""
    ref = max(runs, key=lambda r: r[1])
    rows = lambda arr, name, B: np.ascontiguousarray(arr[:, :B] if name.startswith("saved") else arr[:B])
    others = [r for r in runs if r is not ref]
    bad = []
    for label, B, a in others:
        for name in names:
            x, y = rows(a[name], name, B), rows(ref[2][name], name, B)
            if not same_bits(x, y):              # which rows, and by how much: an edge shows as a run of rows, rounding as scattered ones
                rowwise = np.moveaxis(x.view(np.uint32) != y.view(np.uint32), 1 if name.startswith("saved") else 0, 0)
                d = np.nonzero(rowwise.reshape(B, -1).any(axis=1))[0]
                bad.append((label, name, "against", ref[0], f"{d.size} of {B} rows differ, first {d[:6].tolist()}, last {int(d[-1])}, "
                            f"largest |difference| {float(np.abs(x.astype(np.float64) - y).max()):.3e}"))
    assert not bad, (len(bad), bad[:12])
    assert others and max(B for _, B, _ in others) > more_than, (ref[0], [r[0] for r in others][:3])
    return len(others)


def by_key(got, pick):
    """{key: [(label, B, arrays)]} over all children; pick(child, probe, geo, B, arrays) -> key or None."""
    out = {}
    for c in NAMES:
        for (probe, geo, B), a in split(got[c]).items():
            k = pick(c, probe, geo, B, a)
            if k is not None:
                out.setdefault(k, []).append(((c, probe, geo, B), B, a))
    return out


def test_rows_of_the_bf16x3_forwards_are_the_same_bits(got):
    """z1 of every bf16x3 forward -- latency forms of 16 / 32 / 64 rows, phase-separated with 4 and 8 waves, software-pipelined in its
    five shapes, with and without objective / in-kernel sums -- and the block outputs of those that keep them, at every batch size: the
    first B rows of the geometry's longest run.  The stash words of the complete 32-row tiles at equal B."""
    fam = lambda c, probe, geo, B, a: geo if "z1" in a and probe.startswith(BF16X3) and B <= W.N_SMALL else None
    n = 0
    for geo, runs in by_key(got, fam).items():
        # C3 / nz66 run the pipelined kernel's 256-row form, C5 / tiny / odd / add the phase-separated 8-wave form: 2R + 33 = 545 rows
        n += hold_to_longest(runs, ("z1",), 256)
        # (nz66 keeps block outputs in the latency probes only: 161 rows under ST 4, 97 under ST 2 -- past a 64-row workgroup)
        n += hold_to_longest([r for r in runs if "saved" in r[2]], ("saved",), 64 if geo == "nz66" else 256)
    acts = {}
    for runs in by_key(got, lambda c, probe, geo, B, a: fam(c, probe, geo, B, a) if "act" in a and B >= 32 else None).values():
        for (c, probe, geo, B), _, a in runs:
            t = whole_tiles(a["act"], geo, B)
            # C3 has no padded feature column: its stash is compared across the kernel families too; elsewhere within a family
            first = acts.setdefault((geo, B) if geo == "C3" else (probe[0], geo, B), t)
            assert np.array_equal(t, first), (c, probe, geo, B)
    say(f"bf16x3 rows: {n} runs hold their geometry's longest run's z1 / block-output bits; stash tiles of {len(acts)} (family, geometry, B) agree")
    assert n > 500 and len(acts) > 30


def test_four_and_eight_wave_forms_give_the_same_rows(got):
    """LSNF_FORCE_WAVES 4 against 8.  lsnf_fwd3b_kernel, lsnf_rev3_kernel and lsnf_bwd3_kernel were read for it: in the source the wave
    count enters a wave's first row / tile index, the staging of the weights (Pipe3<NW>), the cooperative copy of the constants, the
    fp16x2 fix-up flag and the order of the batch sums only (csrc/lsnf_rev3.hip: "what a wave computes does not depend on NW").  Held
    to bits across the two forms, on every geometry, every run against the 8-wave run of 545 rows: z1, per-row logdet and the block
    outputs of the phase-separated forward, x / objective_out / ll_out of the bf16x3 throughput reverse and of `sample`, dz and z_new of
    the backward from the stash.
    NOT the forward's per-row ll: measured here, the 4- and the 8-wave code object of lsnf_fwd3b_kernel<1, 1> (geometries `tiny` and
    `add`) give ll one ulp apart on 8 of 128 rows scattered over the batch (19, 22, 27, 33, ...; at most 1.9e-6 absolute at |ll| ~ 16), the same rows
    in every probe, with z1 and logdet equal -- the two objects hold the same count of fp32 instructions (34 mul, 33 fmac, 62 add), so
    what differs is presumably the order in which each sums the squares of -0.5 |z1|^2 (not established further); a rounding
    difference, not an edge of the workgroup.  DESIGN section 2 claims fp32 rounding
    for log-prob across kernels, not bits; ll stays under the float64 gate (2e-6, test_forward_outputs_meet_float64) in both."""
    probes = {"w.phased.plain": ("z1", "logdet"), "w.phased.stash": ("z1", "logdet", "saved"), "w.rev.bf16": ("x", "objout"),
              "w.sample": ("x", "objout", "eps", "ll"), "w.bwd": ("gz",), "w.bwd.lv.tensor": ("z_new",), "w.bwd.lv.philox": ("z_new",)}
    groups = by_key(got, lambda c, probe, geo, B, a: (probe, geo) if probe in probes and B <= W.N_SMALL else None)
    n, bad = 0, []
    for (probe, geo), runs in sorted(groups.items()):
        for name in probes[probe]:               # (each quantity on its own, so that one failure does not hide the others)
            try:
                n += hold_to_longest(runs, (name,), 256)
            except AssertionError as e:
                bad.append(str(e))
    for b in bad:
        say("4 against 8 waves: " + b)
    assert not bad, (len(bad), [b[:300] for b in bad])
    assert len(groups) == 5 * len(probes) and n > 400
    for (probe, geo), runs in groups.items():          # both forms are among the runs of every key
        waves = {dict(W.CHILDREN)[label[0]].get("LSNF_FORCE_WAVES", "4") for label, _, _ in runs}
        assert waves == {"4", "8"}, (probe, geo, waves)


def test_pipelined_shapes_with_32_rows_per_wave_are_the_same_bits(got):
    """LSNF_FWD3Q_SHAPE 242, 82 and 42 keep the same rows per wave: z1, logdet and ll bit for bit (tests/test_gpu_fwd3q_pair.py), every
    run against the 545 rows of shape 82."""
    kids = [n for n, env in W.CHILDREN if env.get("LSNF_FWD3Q_SHAPE") in ("242", "82", "42")]
    assert len(kids) == 3
    groups = by_key(got, lambda c, probe, geo, B, a: (probe, geo) if c in kids and probe in ("q.plain", "q.stats") else None)
    n = sum(hold_to_longest(runs, ("z1", "logdet", "ll"), 256) for runs in groups.values())
    assert len(groups) == 4 and n > 60
    for runs in groups.values():
        assert {label[0] for label, _, _ in runs} == set(kids)


def test_mala_kernels_do_not_depend_on_the_workgroup_shape(got):
    """Everything both MALA calls return, at equal batch size, between children whose kernels really run another ST (the teacher-forced
    inputs of a case are seeded by its batch size, so only equal sizes compare): B = 1, 17 and 97 -- a ragged second 64-row workgroup,
    seven 16-row ones -- in every child, 65 between ST 1 and 4."""
    groups = by_key(got, lambda c, probe, geo, B, a: (probe, geo, B) if probe in ("s.mala", "s.rmala") else None)
    pairs = {}
    for (probe, geo, B), runs in groups.items():
        st = lambda r: W.small3_st(dict(W.CHILDREN)[r[0][0]], geo)[1]
        for r in runs[1:]:
            for name in r[2]:
                assert same_bits(r[2][name], runs[0][2][name]), (r[0], name)
            if st(r) != st(runs[0]):
                pairs[(probe, geo)] = max(pairs.get((probe, geo), 0), B)
    say(f"MALA across ST: largest batch size compared between two different shapes, per (probe, geometry): {pairs}")
    assert len(pairs) == 2 * len(W.MALA_GEOS) and min(pairs.values()) >= 97


def test_stash_keeping_sample_is_the_sample_and_keeps_the_reverses_stash(got):
    """`sample(..., save_for_backward=True, act_saved=)` under every LSNF_SMALL3_ST: x, objective_out, eps and ll are the plain
    sample's bits (flow.sample: "the same launch, same bits"), and the block outputs and the whole 32-row tiles of the stash are those
    that the stash-keeping reverse of the returned eps keeps -- the stash that the reverse-backward probes hold to float64."""
    n = 0
    for c in NAMES:
        cases = split(got[c])
        for (probe, geo, B), a in cases.items():
            if probe != "s.sample.keep":
                continue
            n += 1
            plain = cases[("s.sample", geo, B)]
            for name in ("x", "objout", "eps", "ll"):
                assert same_bits(a[name], plain[name]), (c, geo, B, name)
            assert same_bits(a["x"], a["x_rev"]) and same_bits(a["objout"], a["objout_rev"]), (c, geo, B)
            assert same_bits(a["saved"], a["saved_rev"]), (c, geo, B)
            assert np.array_equal(whole_tiles(a["act"], geo, B), whole_tiles(a["act_rev"], geo, B)), (c, geo, B)
    assert n > 50


def test_in_kernel_draws_do_not_depend_on_the_form(got):
    """`sample`'s eps is a pure function of (seed, offset, row, column): the same bits from every kernel, shape and batch size -- every
    run against its geometry's longest (the 32 769 rows of the fp32 reverse where that runs, 545 elsewhere)."""
    groups = by_key(got, lambda c, probe, geo, B, a: geo if "eps" in a else None)
    n = sum(hold_to_longest(runs, ("eps",), 256 if geo != "nz66" else 64) for geo, runs in groups.items())
    assert len(groups) == len(W.GEOS) and n > 300
