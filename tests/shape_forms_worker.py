"""The case table of tests/test_gpu_shape_forms.py and the child process that runs it (not a test module).

    python tests/shape_forms_worker.py CHILD_NAME OUT.npz

The workgroup-shape knobs of INTEGRATION.md section 4 are read once per process, so every knob setting (CHILDREN) runs in a fresh
child: the parent passes the environment, the child makes the seeded calls of its probe groups through the public Python API and
saves every output tensor into one .npz.  Each probe's name is printed and flushed BEFORE it runs: if a child dies, its last line
names what was running.

Inputs do not depend on the batch size: a case of B rows takes the FIRST B rows of its geometry's seeded master batch
(`oracle.smooth_batch` rows: kink-free, so gradient probes set no row aside), so the float64 oracle is evaluated once per geometry
and the rows of two forms can be compared bit for bit whatever their batch sizes."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import flow_oracle as O  # noqa: E402
import reverse_restated as R  # noqa: E402

# ---- the table ----------------------------------------------------------------------------------------------------------
# every value INTEGRATION.md section 4 documents for a workgroup-shape knob (LSNF_TN_PLAIN: set, whatever the value)
KNOB_VALUES = {"LSNF_FWD3Q_SHAPE": ("41", "81", "42", "82", "242"), "LSNF_SMALL3_ST": ("1", "2", "4"), "LSNF_FORCE_WAVES": ("4", "8"),
               "LSNF_FWD_WAVES": ("4", "8"), "LSNF_TN_PLAIN": ("1",), "LSNF_TN_X3": ("0",), "LSNF_TN_CHUNK": ("16", "4096")}
# The knobs address disjoint kernels, so one child sets several.  LSNF_TN_CHUNK=24 is outside the documented range (not a multiple of
# 16): the fp32 contractions bound every row by the chunk's end and the bf16 one rounds the value up, so it must give the same result.
CHILDREN = [
    ("baseline", {}),
    ("q41_w4_st1_chunk16", {"LSNF_FWD3Q_SHAPE": "41", "LSNF_FORCE_WAVES": "4", "LSNF_FWD_WAVES": "4", "LSNF_SMALL3_ST": "1", "LSNF_TN_CHUNK": "16"}),
    ("q81_w8_st2_chunk4096", {"LSNF_FWD3Q_SHAPE": "81", "LSNF_FORCE_WAVES": "8", "LSNF_FWD_WAVES": "8", "LSNF_SMALL3_ST": "2", "LSNF_TN_CHUNK": "4096"}),
    ("q42_st4_plain", {"LSNF_FWD3Q_SHAPE": "42", "LSNF_SMALL3_ST": "4", "LSNF_TN_PLAIN": "1"}),
    ("q82_x3off", {"LSNF_FWD3Q_SHAPE": "82", "LSNF_TN_X3": "0"}),
    ("q242_chunk24", {"LSNF_FWD3Q_SHAPE": "242", "LSNF_TN_CHUNK": "24"}),
]
GROUP_KNOBS = {"fwd3q": ("LSNF_FWD3Q_SHAPE",), "waves": ("LSNF_FORCE_WAVES", "LSNF_FWD_WAVES"), "small3": ("LSNF_SMALL3_ST",),
               "tn": ("LSNF_TN_PLAIN", "LSNF_TN_X3", "LSNF_TN_CHUNK"),
               "big": ()}                    # no knob: the baseline alone runs it
# (nz, f_width, depth, coupling): <HT, WT> = <2, 2>, <2, 4>, <1, 1>; odd sizes; the 8-byte row path; additive coupling
GEOS = {"C3": (128, 64, 5, 1), "C5": (100, 128, 5, 1), "tiny": (8, 4, 2, 1), "odd": (126, 127, 2, 1), "nz66": (66, 64, 5, 1), "add": (20, 12, 5, 0)}
N_SMALL = 2 * 256 + 33                       # rows of a geometry's master batch: 2R + 33 of the largest workgroup
X3_ROWS = (12288, 12289, 12543)              # csrc/lsnf_layout.h LSNF_X3_MIN_ROWS: the tiled dump and the bf16 contraction start there
LDS_ROWS = (4096, 4097, 4113)                # csrc/lsnf_api.hip select_contraction: the LDS-staged contraction starts there
N_LARGE = max(X3_ROWS)
BIG = 128 * 256 + 1                          # csrc/lsnf_rev.hip: the fp32 throughput reverse has no knob, its 8-wave form runs above 32 768 rows
STEP = 0.1                                   # Langevin step size of the probes (the reference's)
PHILOX = (2 ** 63 + 12345, 77)               # seed, offset of the in-kernel draws


def groups_of(env):
    """The probe groups a child runs: those whose kernels its knobs address; the baseline (no knob) runs all."""
    return [g for g, knobs in GROUP_KNOBS.items() if not env or any(k in env for k in knobs)]


def edge_rows(R):
    """The batch sizes at which a form with R rows per workgroup goes wrong: one row, a second 16-row tile, one short of / equal to /
    one past a workgroup, a ragged third workgroup."""
    return sorted({1, 17, R - 1, R, R + 1, 2 * R + 33})


def fwd3q_rows(env):
    """Rows per workgroup of lsnf_fwd3q_kernel (csrc/lsnf_fwd3p.hip lsnf_launch_forward3q): (plain form, stash / dump form).  Code
    NS = N waves of 16 * S rows (242: the 42 shape, two workgroups per CU); below 32 768 rows the default is 41; the stash and dump
    forms have 32 rows per wave and 8 waves under code 82 only."""
    code = env.get("LSNF_FWD3Q_SHAPE", "41")
    waves, st = int(code[-2]), int(code[-1])
    return 16 * st * waves, (256 if code == "82" else 128)


def waves_rows(env):
    """Rows per workgroup (32 per wave) of the bf16 throughput kernels (csrc/lsnf_launch.h lsnf_eight_waves) and of the fp32
    throughput forward (csrc/lsnf_fwd.hip); 4 waves below 32 768 rows."""
    return 32 * int(env.get("LSNF_FORCE_WAVES", "4")), 32 * int(env.get("LSNF_FWD_WAVES", "4"))


def small3_st(env, geo):
    """(ST wanted, ST the kernels really run) for the latency kernels, 16 * ST rows per workgroup (csrc/lsnf_launch.h
    lsnf_small3_st_wanted; below 4 096 rows the default is 1).  lsnf_small3_*_st: a shape that is not instantiated, or whose LDS does
    not fit, gives way to the next smaller one -- the <2, 4> geometry (f_width 128) has ST = 1 and 2 only."""
    want = int(env.get("LSNF_SMALL3_ST", "1"))
    return want, (min(want, 2) if geo_of(geo)[1] > 64 else want)


def small3_rows(env, geo):
    want, got = small3_st(env, geo)
    return sorted(set(edge_rows(16 * want)) | set(edge_rows(16 * got)))


def tn_rows(env):
    """Batch sizes of the parameter-gradient probes: around one chunk of the plain contraction (128 rows by default, LSNF_TN_CHUNK
    otherwise; 4 096: a single chunk), the sizes at which the LDS-staged and the bf16 contraction start.  With LSNF_TN_CHUNK = 16 and
    4 096 the large sizes end in chunks of 1 and 17 rows."""
    chunk = int(env.get("LSNF_TN_CHUNK", "128"))
    return edge_rows(min(chunk, 128)), LDS_ROWS, X3_ROWS


# The MALA probes: three geometries of GEOS, and from tests/chain_geometries.py a ragged half (33) and a second half-tile that is
# entirely padding, both <2, 2>.  The two are kept out of GEOS, whose sorted order seeds the inputs of every other probe.
CHAIN_GEOS = {"half33": (66, 33, 2, 1), "pad10": (10, 40, 2, 1)}
MALA_GEOS = ("C3", "C5", "tiny") + tuple(CHAIN_GEOS)


def geo_of(name):
    return GEOS[name] if name in GEOS else CHAIN_GEOS[name]


def mala_rows(env, geo):
    """The MALA cases are seeded by their batch size, so two shapes compare at equal sizes only: 97 rows (past a 64-row workgroup, a
    ragged seventh 16-row one) run under every shape."""
    return sorted(set(edge_rows(16 * small3_st(env, geo)[1])) | {97})


def params_of(geo):
    nz, w, depth, coupling = GEOS[geo]
    p = O.init_params(nz, w, depth, seed=40 + sorted(GEOS).index(geo))
    if coupling == 0:                        # additive: fc_zeros maps to the nz/2 shifts only (model.py:385)
        p = {k: (v[:, : v.shape[1] // 2].contiguous() if ".f.fc_zeros." in k else v) for k, v in p.items()}
    return p


@functools.lru_cache(maxsize=None)
def master(geo, n=N_SMALL):
    """Seeded inputs of n rows (CPU, fp32): z (smooth_batch), objective, eps = f_fp64(z) (a kink-free input of the REVERSE, as
    tests/test_gpu_reverse_autograd.py kinkfree_case), upstream gradients g_x / g_o, Langevin noise and the generator's gradient."""
    nz = GEOS[geo][0]
    p = params_of(geo)
    seed = 9000 + 10 * sorted(GEOS).index(geo) + (n != N_SMALL)
    z, _ = O.smooth_batch(p, n, nz, seed=seed)
    g = torch.Generator().manual_seed(seed + 5)
    m = {"z": z, "obj": torch.randn(n, generator=g), "gx": torch.randn(n, nz, generator=g), "go": torch.randn(n, generator=g),
         "noise": torch.randn(n, nz, generator=g), "gg": 0.1 * torch.randn(n, nz, generator=g)}
    m["eps"] = R.forward64(p, z)[0].float()
    return p, m


@functools.lru_cache(maxsize=None)
def big_inputs(geo):
    """(eps, objective) of BIG seeded rows for the reverse."""
    g = torch.Generator().manual_seed(7000 + sorted(GEOS).index(geo))
    return torch.randn(BIG, GEOS[geo][0], generator=g), torch.randn(BIG, generator=g)


def key(probe, geo, B, arr):
    return f"{probe}|{geo}|B{B}|{arr}"


# ---- the child ----------------------------------------------------------------------------------------------------------
class Child:
    def __init__(self, env):
        import lsnf_amd
        self.L, self.F, self.env = lsnf_amd, lsnf_amd.flow, env
        self.dev = torch.device("cuda:0")
        self.res = {}
        self.plans = {}

    def plan(self, geo):
        if geo not in self.plans:
            nz, w, depth, coupling = GEOS[geo]
            params = self.F.params_from_state_dict(params_of(geo), depth, self.dev)
            self.plans[geo] = (self.F.prepare(params, nz, w, depth, coupling), params)
        return self.plans[geo]

    def mode(self, small, math):
        self.F.set_small_batch_max(small)
        self.F.set_math_mode(getattr(self.F, math))

    def rows(self, geo, B, *names, n=N_SMALL):
        m = master(geo, n)[1]
        return [m[k][:B].contiguous().to(self.dev) for k in names]

    def put(self, probe, geo, B, **arrays):
        torch.cuda.synchronize()
        for name, t in arrays.items():
            if t is not None:
                a = t.detach().cpu().contiguous()
                if name == "guard":              # (min, max): both 7.0 if no word was touched; a NaN written there shows in either
                    a = torch.stack([a.min(), a.max()])
                self.res[key(probe, geo, B, name)] = (a.view(torch.int32) if name.startswith("act") else a).numpy()

    def start(self, probe, geo, B):
        print(f"probe {probe} {geo} B={B}", flush=True)

    def nan(self, *shape):
        return torch.full(shape, float("nan"), device=self.dev)

    def guard(self):
        return torch.full((4096,), 7.0, device=self.dev)     # allocated behind the outputs: a store past the batch would land here

    # -- forward: every output NaN-filled first, a sentinel buffer behind them
    def forward(self, probe, geo, B, *, objective=False, stats=False, act=False, saved=False, n=N_SMALL):
        self.start(probe, geo, B)
        plan, _ = self.plan(geo)
        z, obj = self.rows(geo, B, "z", "obj", n=n)
        depth = GEOS[geo][2]
        out = (self.nan(B, plan.nz), self.nan(B), self.nan(B))
        a = self.F.new_act_saved(plan, B, self.dev).fill_(float("nan")) if act else None
        s = self.nan(depth - 1, B, plan.nz) if saved and depth > 1 else None
        st = self.F.new_stats(self.dev) if stats else None
        g = self.guard()
        self.F.forward(plan, z, obj if objective else None, out=out, stats=st, act_saved=a, z_saved_out=s)
        self.put(probe, geo, B, z1=out[0], logdet=out[1], ll=out[2], act=a, saved=s, sums=None if st is None else st[4:7], guard=g)
        return z, out, s, a

    def reverse(self, probe, geo, B, keep=False):
        self.start(probe, geo, B)
        plan, _ = self.plan(geo)
        eps, obj = [t.to(self.dev) for t in big_inputs(geo)] if B == BIG else self.rows(geo, B, "eps", "obj")
        out = (self.nan(B, plan.nz), self.nan(B))
        g = self.guard()
        if not keep:
            self.F.reverse(plan, eps, obj, out=out)
            self.put(probe, geo, B, x=out[0], objout=out[1], guard=g)
            return None
        act = self.F.new_act_saved(plan, B, self.dev).fill_(float("nan"))
        saved = self.nan(GEOS[geo][2] - 1, B, plan.nz)
        self.F.reverse(plan, eps, obj, out=out, act_saved=act, z_saved_out=saved)
        self.put(probe, geo, B, x=out[0], objout=out[1], act=act, saved=saved, guard=g)
        return eps, saved, act

    def sample(self, probe, geo, B):
        self.start(probe, geo, B)
        plan, _ = self.plan(geo)
        out = (self.nan(B, plan.nz), self.nan(B), self.nan(B, plan.nz), self.nan(B))
        g = self.guard()
        self.F.sample(plan, B, self.F.PhiloxNoise(*PHILOX, 3), out=out)
        self.put(probe, geo, B, x=out[0], objout=out[1], eps=out[2], ll=out[3], guard=g)

    def sample_keep(self, probe, geo, B):
        """The stash-keeping sample, then the stash-keeping reverse of the eps it returned: the same kernel without the draw."""
        self.start(probe, geo, B)
        plan, _ = self.plan(geo)
        out = (self.nan(B, plan.nz), self.nan(B), self.nan(B, plan.nz), self.nan(B))
        act = self.F.new_act_saved(plan, B, self.dev).fill_(float("nan"))
        g = self.guard()
        saved = self.F.sample(plan, B, self.F.PhiloxNoise(*PHILOX, 3), out=out, save_for_backward=True, act_saved=act)[4]
        act2 = self.F.new_act_saved(plan, B, self.dev).fill_(float("nan"))
        saved2 = self.nan(GEOS[geo][2] - 1, B, plan.nz)
        x2, obj2, _ = self.F.reverse(plan, out[2], None, act_saved=act2, z_saved_out=saved2)
        self.put(probe, geo, B, x=out[0], objout=out[1], eps=out[2], ll=out[3], saved=saved, act=act, guard=g, x_rev=x2, objout_rev=obj2,
                 saved_rev=saved2, act_rev=act2)

    def backward(self, probe, geo, B):
        """backward_z from the forward's stash, then the Langevin tail with tensor and with Philox noise."""
        z, out, saved, act = self.forward(probe + ".fwd", geo, B, act=True, saved=True)
        plan, _ = self.plan(geo)
        self.start(probe, geo, B)
        gz = self.F.backward_z(plan, out[0], saved, ll_scale=-1.0, act_saved=act)
        self.put(probe, geo, B, gz=gz)
        noise, gg = self.rows(geo, B, "noise", "gg")
        for how, xi in (("tensor", noise), ("philox", self.F.PhiloxNoise(*PHILOX, 3))):
            self.start(f"{probe}.lv.{how}", geo, B)
            z_new, ll, gf, ggn = self.F.langevin_step(plan, z, gg, xi, STEP)
            self.put(f"{probe}.lv.{how}", geo, B, z_new=z_new, ll=ll, gf=gf, ggn=ggn)

    def reverse_backward(self, probe, geo, B):
        """reverse_backward_z and reverse_langevin_step from the stash the keeping reverse left."""
        eps, saved, act = self.reverse(probe + ".keep", geo, B, keep=True)
        plan, _ = self.plan(geo)
        gx, go, noise = self.rows(geo, B, "gx", "go", "noise")
        self.start(probe, geo, B)
        self.put(probe, geo, B, geps=self.F.reverse_backward_z(plan, eps, saved, act, gx, go),
                 geps_x=self.F.reverse_backward_z(plan, eps, saved, act, gx, None))      # (the step below has no g_obj)
        self.start(probe + ".lv", geo, B)
        e_new, g, gn, en = self.F.reverse_langevin_step(plan, eps, saved, act, gx, noise, STEP, want_g=True)
        self.put(probe + ".lv", geo, B, eps_new=e_new, g=g, gn=gn, en=en)

    def params(self, probe, geo, B, n=N_SMALL, keep_rows=False):
        """backward_params on the fast path (forward with stash and h dump, NaN-filled first) and on the recomputing path."""
        plan, params = self.plan(geo)
        (z,) = self.rows(geo, B, "z", n=n)
        F, depth = self.F, GEOS[geo][2]
        self.start(probe + ".fast", geo, B)
        act = F.new_act_saved(plan, B, self.dev).fill_(float("nan"))
        ws = F.new_params_workspace(plan, B, self.dev).fill_(float("nan"))
        saved = self.nan(depth - 1, B, plan.nz) if depth > 1 else None
        g = self.guard()
        z1, _, ll, _ = F.forward(plan, z, act_saved=act, z_saved_out=saved, params_ws=ws)
        _, gz, flat = F.backward_params(plan, params, z, z1, saved, ll_scale=-1.0 / B, want_grad_z=True, want_flat=True, act_saved=act, workspace=ws)
        self.put(probe + ".fast", geo, B, flat=flat, gz=gz if keep_rows or B <= N_SMALL else None, z1=z1 if keep_rows else None,
                 ll=ll if keep_rows else None, guard=g)
        self.start(probe + ".slow", geo, B)
        z1b, _, _, savedb = F.forward(plan, z, want_ll=False, save_for_backward=True)
        _, gzb, flatb = F.backward_params(plan, params, z, z1b, savedb, ll_scale=-1.0 / B, want_grad_z=True, want_flat=True)
        self.put(probe + ".slow", geo, B, flat=flatb, gz=gzb if B <= N_SMALL else None)

    def mala(self, geo, B):
        """The teacher-forced first step of tests/test_gpu_mala.py and tests/test_gpu_rmala.py (their Case / run), tensor noise."""
        import test_gpu_mala as ZM
        import test_gpu_rmala as RMt
        for probe, T in (("s.mala", ZM), ("s.rmala", RMt)):
            self.start(probe, geo, B)
            s = T.Setup(self.L, self.dev, *geo_of(geo), B, "default")
            st = s.c.steps[0]
            r = T.run(self.L, s, st, st.noise.to(self.dev), st.u.to(self.dev))
            state, out = r[0], r[-1]
            names = ("z_next", "acc", "la", "ll")[: len(out)]
            self.put(probe, geo, B, state_z=state.z, state_grad=state.grad, state_energy=state.energy, **dict(zip(names, out)))

    # -- the groups
    def run_fwd3q(self):
        self.mode(0, "MATH_BF16X3")
        plain, stash = fwd3q_rows(self.env)
        for geo in ("C3", "nz66"):
            for B in sorted(set(edge_rows(plain)) | set(edge_rows(stash))):
                self.forward("q.plain", geo, B)
                self.forward("q.stats", geo, B, objective=True, stats=True)
                if geo == "C3":
                    self.forward("q.act", geo, B, act=True)
                    self.forward("q.saved", geo, B, saved=True)
                    self.forward("q.act_saved", geo, B, act=True, saved=True)
        for B in X3_ROWS:                    # the STASH = 2 instantiation: the tiled h dump, read by the bf16 contraction
            self.params("q.ws", "C3", B, n=N_LARGE, keep_rows=True)

    def run_waves(self):
        bf16, fp32 = waves_rows(self.env)
        for geo in ("C3", "C5", "tiny", "odd", "add"):
            for B in sorted(set(edge_rows(bf16)) | set(edge_rows(fp32))):
                for name, math in (("fp32", "MATH_FP32"), ("phased", "MATH_BF16X3_PHASED"), ("fp16", "MATH_FP16X2")):
                    self.mode(0, math)
                    self.forward(f"w.{name}.plain", geo, B)
                    self.forward(f"w.{name}.stash", geo, B, act=True, saved=True)
                for name, math in (("bf16", "MATH_BF16X3"), ("fp16", "MATH_FP16X2")):
                    self.mode(0, math)
                    self.reverse(f"w.rev.{name}", geo, B)
                self.mode(0, "MATH_FP16X2")
                self.sample("w.sample.fp16", geo, B)
                self.mode(0, "MATH_BF16X3")
                self.sample("w.sample", geo, B)
                self.backward("w.bwd", geo, B)
                if geo in ("C3", "C5", "tiny"):
                    self.mode(0, "MATH_BF16X3_PHASED")
                    self.params("w.params", geo, B)
        self.mode(0, "MATH_BF16X3_PHASED")   # the phase-separated forward and the backward with the tiled dump, 4 or 8 waves
        for B in X3_ROWS:
            self.params("w.params", "C3", B, n=N_LARGE)

    def run_small3(self):
        self.mode(1 << 30, "MATH_BF16X3")
        for geo in GEOS:
            print("small3 %s: LSNF_SMALL3_ST wanted %d, runs %d" % ((geo,) + small3_st(self.env, geo)), flush=True)
        for geo in GEOS:
            for B in small3_rows(self.env, geo):
                self.forward("s.fwd.plain", geo, B)
                self.forward("s.fwd.stats", geo, B, objective=True, stats=True)
                self.reverse("s.rev", geo, B)
                self.sample("s.sample", geo, B)
                self.sample_keep("s.sample.keep", geo, B)
                self.backward("s.bwd", geo, B)
                self.reverse_backward("s.rbwd", geo, B)
                if geo in ("C3", "C5", "tiny"):
                    self.params("s.params", geo, B)
        for geo in MALA_GEOS:
            for B in mala_rows(self.env, geo):
                self.mala(geo, B)

    def run_big(self):
        """The 8-wave forms of the fp32 throughput reverse (plain and sampling): reached through the batch size alone."""
        self.mode(0, "MATH_FP32")
        for geo in ("C3", "C5", "tiny"):
            if geo != "C3":                  # (the suite's large-batch tests run the <2, 2> plain form)
                self.reverse("b.rev.fp32", geo, BIG)
            self.sample("b.sample.fp32", geo, BIG)

    def run_tn(self):
        small, lds, x3 = tn_rows(self.env)
        self.mode(self.F.SMALL_BATCH_AUTO, "MATH_BF16X3")
        for B in tuple(small) + lds:
            self.params("t.auto", "C3", B, n=N_LARGE if B > N_SMALL else N_SMALL)
        self.mode(0, "MATH_BF16X3")
        for B in x3:
            self.params("t.thr", "C3", B, n=N_LARGE)


def main():
    name, out = sys.argv[1], sys.argv[2]
    env = dict(CHILDREN)[name]
    for knobs in GROUP_KNOBS.values():       # the environment is the parent's to pass: refuse to run under another one
        for k in knobs:
            assert os.environ.get(k) == env.get(k), (k, os.environ.get(k), env.get(k))
    child = Child(env)
    for group in groups_of(env):
        print(f"group {group}", flush=True)
        getattr(child, "run_" + group)()
    torch.cuda.synchronize()
    np.savez(out, **child.res)
    print(f"child {name} ok: {len(child.res)} arrays", flush=True)


if __name__ == "__main__":
    main()
