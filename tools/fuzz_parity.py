"""Randomised parity sweep (GPU box): random geometries x batch sizes at the kernel-family / tile boundaries x every
entry point x every arithmetic mode x affine / additive coupling, each checked against the float64 oracle; every case also
draws one documented call form of the ABI (forward and reverse in place, the stack in two pieces sharing one activation stash,
one row tensor of the forward at a 4- or 8-byte offset) from a second generator, so that the geometries of a seed do not depend
on the forms.  Batches are kink-free (no row within 2e-5
of a ReLU kink, kink_free_batch), so every row's gradients and the parameter gradients of every case -- recomputing path, and fast
path in the bf16x3-family modes -- are held to the oracle.  Prints one line per failing case and a summary; exit code 1 if
anything failed.  `python tools/fuzz_parity.py [n_cases] [seed]`.
The oracle is the checker only (tests/ infrastructure); the product path is the C ABI."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import lsnf_amd
from lsnf_amd import flow
from oracle import flow_oracle as O, philox_oracle as PO

dev = torch.device("cuda:0")
BATCHES = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 255, 257, 1000, 4097, 5003, 8193, 9001, 16384, 16385, 32768, 32769]
fails, checks = [], 0


def rel(a, b):
    return float((a.double().cpu() - b.double()).abs().max() / max(1e-30, float(b.double().abs().max())))


def check(tag, name, got, ref, tol):
    global checks
    checks += 1
    e = rel(got, ref)
    if not (e <= tol) or not bool(torch.isfinite(got).all()):
        fails.append((tag, name, e, tol))
        print("FAIL", tag, name, "err %.3g > %.3g" % (e, tol), flush=True)


def kink_free_batch(p, B, nz, seed, margin=2e-5):
    """B seeded N(0,1) rows with every row whose ReLU margin is <= `margin` redrawn from the same generator: what
    oracle.smooth_batch returns, restated here on oracle.relu_margin alone because tests/test_gpu_fuzz.py runs this tool
    beside whichever oracle/ the test tree brings, and earlier ones have no smooth_batch."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, nz, generator=g)
    bad = torch.nonzero(O.relu_margin(p, z) <= margin).flatten()
    while bad.numel():
        z[bad] = torch.randn(int(bad.numel()), nz, generator=g)
        bad = bad[O.relu_margin(p, z[bad]) <= margin]
    return z


def offset_view(shape, off, src=None):
    """A contiguous tensor `off` floats past a 16-byte boundary (a view into a larger allocation), optionally a copy of src."""
    n = int(np.prod(shape))
    t = torch.empty(n + 4, dtype=torch.float32, device=dev)[off: off + n].view(shape)
    assert t.data_ptr() % 16 == 4 * off
    return t if src is None else t.copy_(src)


def nan_stash(plan, B, n_saved):
    act = flow.new_act_saved(plan, B, dev)
    act.fill_(float("nan"))
    saved = torch.full((n_saved, B, plan.nz), float("nan"), device=dev) if n_saved > 0 else None
    return act, saved


def call_form(tag, form, plan, zd, od, cut, mis_tensor, mis_off, ref):
    """One documented call form of the ABI (include/lsnf_flow.h) per case, in the math mode / threshold in force, against
    the same oracle and tolerances as the plain calls."""
    B, depth = zd.shape[0], plan.depth
    ld_ref, ll_ref = ref["ld"] + ref["obj"], ref["ll"] + ref["obj"]
    ld_tol = 1e-5 if ld_ref.abs().max() > 1 else 1e-3
    if form == "inplace":                      # z_out == z_in, logdet_out == objective; reverse: the same two aliases
        zc, oc = zd.clone(), od.clone()
        ll = torch.empty(B, device=dev)
        flow.forward(plan, zc, oc, out=(zc, oc, ll))
        check(tag, "z1", zc, ref["z1"], 2e-5)
        check(tag, "logdet", oc, ld_ref, ld_tol)
        check(tag, "ll", ll, ll_ref, 1e-5)
        zc, oc = zd.clone(), od.clone()
        flow.reverse(plan, zc, oc, out=(zc, oc))
        check(tag, "reverse_x", zc, ref["x"], 5e-5)
        check(tag, "reverse_obj", oc, ref["xobj"], 2e-5)
        return
    if form == "split":                        # [0, cut) + [cut, depth): one stash (indexed by absolute block), z_saved per piece
        cut = min(cut, depth)
        act, _ = nan_stash(plan, B, 0)
        z, ld, ll, outs = zd, od, None, []
        for a, b in ((0, cut), (cut, depth)):
            if b > a:
                _, sv = nan_stash(plan, B, b - a - 1)
                z, ld, ll, _ = flow.forward(plan, z, ld, first_block=a, n_blocks=b - a, act_saved=act, z_saved_out=sv)
                outs += ([] if sv is None else list(sv)) + [z]
        z1, saved = z, (torch.stack(outs[:-1]) if depth > 1 else None)
    else:                                      # one row tensor of the forward 4 or 8 bytes off a 16-byte boundary
        act, saved = nan_stash(plan, B, depth - 1)
        z_in = offset_view(zd.shape, mis_off if mis_tensor == "z_in" else 0, zd)
        z1 = offset_view(zd.shape, mis_off if mis_tensor == "z_out" else 0)
        if saved is not None:
            saved = offset_view(saved.shape, mis_off if mis_tensor == "z_saved" else 0, saved)
        ld, ll = torch.empty(B, device=dev), torch.empty(B, device=dev)
        flow.forward(plan, z_in, od, out=(z1, ld, ll), act_saved=act, z_saved_out=saved)
    check(tag, "z1", z1, ref["z1"], 2e-5)
    check(tag, "logdet", ld, ld_ref, ld_tol)
    check(tag, "ll", ll, ll_ref, 1e-5)
    check(tag, "grad_z", flow.backward_z(plan, z1, saved, ll_scale=-1.0, act_saved=act), ref["gz"], 2e-4)


def run(n_cases, seed, batches=BATCHES):
    """Returns (number of checks, list of failures (tag, quantity, error, tolerance))."""
    global checks
    del fails[:]
    checks = 0
    rs = np.random.RandomState(seed)
    rs2 = np.random.RandomState(seed + 7919)      # coupling type and call form: a stream of its own, so that `rs` draws what it always drew
    t00 = time.time()
    prev_small, prev_mode = flow.set_small_batch_max(flow.SMALL_BATCH_AUTO), flow.set_math_mode(-1)   # (restored below)
    try:
        for case in range(n_cases):
            nz = 2 * int(rs.randint(1, 65))
            width = int(rs.choice([int(rs.randint(1, 129)), 32, 64, 128, 33, 65, 96]))
            depth = int(rs.randint(1, 7))
            B = int(rs.choice(batches))
            small_max = int(rs.choice([0, 16384]))          # 0: throughput family for every B; default: latency family here
            p32 = O.init_params(nz, width, depth, seed=1000 + case, fcz_std=0.05, all_std=float(rs.choice([0.0, 0.02])))
            coupling = int(rs2.randint(0, 2))
            form = str(rs2.choice(["inplace", "split", "misaligned"]))
            cut = int(rs2.randint(1, max(depth, 2)))                       # split: blocks [0, cut) + [cut, depth)
            mis_tensor, mis_off = str(rs2.choice(["z_in", "z_out", "z_saved"])), int(rs2.choice([1, 2]))
            if coupling == 0:                    # additive: fc_zeros maps to the nz/2 shifts only (model.py:385)
                for i in range(depth):
                    for k in ("f.fc_zeros.w", "f.fc_zeros.b", "f.fc_zeros.logs"):
                        p32[O.block_prefix(i) + k] = p32[O.block_prefix(i) + k][:, : nz // 2].contiguous()
            p64 = O.to_dtype(p32, torch.float64)
            z = kink_free_batch(p32, B, nz, seed=case)         # every row away from a ReLU kink (gradients are discontinuous there)
            obj0 = torch.randn(B, generator=torch.Generator().manual_seed(case + 7)).float()
            gg = torch.randn(B, nz, generator=torch.Generator().manual_seed(case + 11)).float()
            noise_t = torch.randn(B, nz, generator=torch.Generator().manual_seed(case + 13)).float()
            step = float(rs.choice([0.1, 0.3]))
            z1_ref, ld_ref, ll_ref = O.flow_log_prob(p64, z.double(), coupling)
            gz_ref = O.grad_neg_sum_ll_wrt_z(p64, z.double(), coupling)
            x_ref, xobj_ref = O.flow_reverse(p64, z.double(), obj0.double(), coupling)
            gp_ref = O.grad_neg_mean_ll_wrt_params(p64, z.double(), coupling)
            params = flow.params_from_state_dict(p32, depth, dev)
            try:
                plan = flow.prepare(params, nz, width, depth, coupling)
            except lsnf_amd.LsnfError as e:
                print("unsupported geometry", nz, width, depth, e)
                continue
            zd, od = z.to(dev), obj0.to(dev)
            flow.set_small_batch_max(small_max)
            for mode in (flow.MATH_FP32, flow.MATH_BF16X3, flow.MATH_BF16X3_PHASED, flow.MATH_FP16X2):
                flow.set_math_mode(mode)
                tag = f"case{case} nz={nz} w={width} d={depth} c={coupling} B={B} small_max={small_max} mode={mode}"
                for stash in (False, True):
                    act = flow.new_act_saved(plan, B, dev) if stash else None
                    z1, ld, ll, saved = flow.forward(plan, zd, None, want_ll=True, save_for_backward=True, act_saved=act)
                    t = tag + (" stash" if stash else "")
                    check(t, "z1", z1, z1_ref, 2e-5)
                    check(t, "logdet", ld, ld_ref if ld_ref.abs().max() > 1e-3 else ld_ref + 1.0 - 1.0, 1e-5 if ld_ref.abs().max() > 1 else 1e-3)
                    check(t, "ll", ll, ll_ref, 1e-5)
                    gz = flow.backward_z(plan, z1, saved, ll_scale=-1.0, act_saved=act)
                    check(t, "grad_z", gz, gz_ref, 2e-4)
                # Langevin step (train.py:316-329) with explicit noise and with in-kernel Philox noise (oracle/philox_oracle.py)
                for kind in ("tensor", "philox"):
                    if kind == "tensor":
                        nref = noise_t
                        zn, ll2, gfn, ggn = flow.langevin_step(plan, zd, gg.to(dev), noise_t.to(dev), step)
                    else:
                        ph = flow.PhiloxNoise(seed=1234 + case, offset=5 + case)
                        nref = torch.from_numpy(PO.langevin_noise(B, nz, 1234 + case, 5 + case, 0)).float()
                        zn, ll2, gfn, ggn = flow.langevin_step(plan, zd, gg.to(dev), ph, step)
                    zn_ref = z.double() - 0.5 * step * step * (gg.double() + gz_ref) + step * nref.double()
                    check(tag, "langevin_z_" + kind, zn, zn_ref, 2e-5)
                    check(tag, "langevin_ll_" + kind, ll2, ll_ref, 1e-5)
                x, xo = flow.reverse(plan, zd, od)
                check(tag, "reverse_x", x, x_ref, 5e-5)
                check(tag, "reverse_obj", xo, -xobj_ref, 2e-5)     # the oracle returns -objective like the reference (model.py:498)
                # round trip through the product path alone
                z1, ld, _, _ = flow.forward(plan, zd, od, want_ll=False)
                zb, ob = flow.reverse(plan, z1, ld)
                check(tag, "roundtrip_z", zb, z.double(), 5e-5)
                check(tag, "roundtrip_obj", ob, obj0.double() if B > 1 or abs(float(obj0[0])) > 1e-2 else ob.double().cpu(), 5e-4)
                call_form(tag + " " + form, form, plan, zd, od, cut, mis_tensor, mis_off,
                          dict(z1=z1_ref, ld=ld_ref, ll=ll_ref, gz=gz_ref, x=x_ref, xobj=-xobj_ref, obj=obj0.double()))
                # parameter gradients: the recomputing path, and in the bf16x3-family modes also the fast path (the forward keeps
                # the stash and writes h1 / h2 into the workspace, the backward runs from them)
                keys = [O.block_prefix(i) + k for i in range(depth) for k in flow.BLOCK_PARAM_KEYS]
                for fast in ((False, True) if flow.params_fast_path() else (False,)):
                    act = flow.new_act_saved(plan, B, dev) if fast else None
                    ws = flow.new_params_workspace(plan, B, dev) if fast else None
                    z1, _, _, saved = flow.forward(plan, zd, None, want_ll=False, save_for_backward=True, act_saved=act, params_ws=ws)
                    grads = flow.backward_params(plan, params, zd, z1, saved, ll_scale=-1.0 / B, act_saved=act, workspace=ws)
                    for k, g in zip(keys, grads):
                        ref = gp_ref[k].reshape(g.shape)
                        if float(ref.abs().max()) < 1e-6:
                            continue
                        check(tag + (" fast" if fast else ""), "dparam " + k, g, ref, 1e-4)
            print(f"case {case} done: nz={nz} w={width} d={depth} c={coupling} {form} B={B} small_max={small_max}  ({checks} checks, {len(fails)} failures, "
                  f"{time.time() - t00:.0f} s)", flush=True)

    finally:
        flow.set_small_batch_max(prev_small)
        flow.set_math_mode(prev_mode)
    return checks, list(fails)


if __name__ == "__main__":
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    n, bad = run(n_cases, seed)
    print(f"SUMMARY: {n} checks over {n_cases} cases, {len(bad)} failures")
    sys.exit(1 if bad else 0)
