"""CPU: the differentiable reverse pass without a GPU -- the new ABI entry point is declared / exported / bound, validates its
arguments before any HIP call, the plan only grew; the two identities the autograd bridge relies on hold on the float64 oracle;
and the module's reverse no longer refuses tensors that require grad (CPU tensors still fail loudly)."""
import os
import re
import types

import pytest
import torch

from conftest import ROOT, load_golden
from oracle import flow_oracle as O
import reverse_restated as R

import lsnf_amd

LSNF_OK, LSNF_E_ARG, LSNF_E_GEOMETRY = 0, -1, -2


def hps(width=64, depth=5, coupling=1):
    return types.SimpleNamespace(f_n_levels=1, f_depth=depth, f_flow_permutation=2, f_width=width, f_flow_coupling=coupling)


def test_symbol_is_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+lsnf_reverse_backward_z\s*\(", hdr)
    lib = lsnf_amd.load_library()
    assert hasattr(lib, "lsnf_reverse_backward_z")
    assert "lsnf_reverse_backward_z" in lsnf_amd.exported_symbols()
    assert lib.lsnf_abi_version() == 5                          # a symbol was added, nothing else changed
    assert callable(lsnf_amd.flow.reverse_backward_z) and lsnf_amd.reverse_backward_z is lsnf_amd.flow.reverse_backward_z


def test_argument_validation_runs_before_any_hip_call():
    lib = lsnf_amd.load_library()
    call = lambda nz, w, d, c, B: lib.lsnf_reverse_backward_z(None, nz, w, d, c, B, None, None, None, None, None, None, None)
    assert call(130, 64, 5, 1, 4) == LSNF_E_GEOMETRY and call(7, 4, 5, 1, 4) == LSNF_E_GEOMETRY
    assert call(128, 64, 17, 1, 4) == LSNF_E_GEOMETRY and call(128, 64, 5, 2, 4) == LSNF_E_GEOMETRY
    assert call(128, 64, 5, 1, -1) == LSNF_E_ARG
    assert b"lsnf_reverse_backward_z" in lib.lsnf_last_error()
    assert call(128, 64, 5, 1, 0) == LSNF_OK                    # empty batch: nothing to launch, NULL pointers allowed
    assert call(128, 64, 5, 1, 4) == LSNF_E_ARG                 # NULL plan / tensors
    assert call(2, 1, 1, 0, 0) == LSNF_OK and call(126, 127, 16, 1, 0) == LSNF_OK


def test_plan_grew_and_keeps_the_geometry_relations():
    lib = lsnf_amd.load_library()
    assert lib.lsnf_plan_floats(128, 64, 5, 1) > 5 * 32768
    assert lib.lsnf_plan_floats(130, 64, 5, 1) == 0 and lib.lsnf_plan_floats(7, 4, 5, 1) == 0
    assert lib.lsnf_plan_floats(128, 64, 17, 1) == 0
    assert lib.lsnf_plan_floats(128, 64, 5, 0) == lib.lsnf_plan_floats(128, 64, 5, 1) and lib.lsnf_plan_floats(128, 64, 5, 2) == 0
    # the transposed inverse panels: three bf16 matrices of (64 * HT)^2 per block = 1536 * NZT^2 floats, behind the guard words
    # (regions are padded to 256 floats; this one's size is a multiple of 256, so a block more costs exactly one more panel set
    # on top of what it cost before: per block and geometry the other regions are unchanged)
    per_block = lambda nz, w: lib.lsnf_plan_floats(nz, w, 2, 1) - lib.lsnf_plan_floats(nz, w, 1, 1)
    old_per_block_c3 = (1024 * (16 + 4 + 4 + 8) + 32 * 12 + 32) + (1024 * 16 + 32 * 4) + 1024 * (8 + 4 + 4 + 16) + 128 * 128 \
        + 1536 * (16 + 4 + 4 + 8) + 1536 * (8 + 4 + 4 + 16) + 1536 * 16 + 1024 * (16 + 4 + 4 + 8) + 1024 * 16
    assert abs(per_block(128, 64) - (old_per_block_c3 + 1536 * 16)) < 8 * 256     # (only alignment padding besides)


FIXTURES = ["tiny_nz8_w4_B37_trained", "additive_nz20_w12_B33", "c3_nz128_w64_B200", "c5_nz100_w128_B33_trained02"]


@pytest.mark.parametrize("name", FIXTURES)
def test_the_two_identities_hold_on_the_float64_oracle(name):
    """What the bridge relies on: (1) the block recurrence of the new kernel IS the gradient of O.flow_reverse w.r.t. its input,
    and J_f^T g_eps + g_o grad logdet = g_x; (2) the parameter gradients of the reverse are those of the FORWARD at x with
    upstream (-g_eps, -g_o).  float64, <= 1e-9 relative."""
    p, g = load_golden(name)
    eps = torch.from_numpy(g["rev_in"]).double()
    B, nz = eps.shape
    gen = torch.Generator().manual_seed(7)
    gx = torch.randn(B, nz, generator=gen, dtype=torch.float64)
    go = torch.randn(B, generator=gen, dtype=torch.float64)
    obj = torch.randn(B, generator=gen, dtype=torch.float64)
    x, _, g_eps, g_theta = R.reverse_loss_grads(p, eps, obj, gx, go, torch.float64, want_params=True)
    # (1) the recurrence, and the adjoint form of the same statement through the FORWARD's autograd
    rec = R.reverse_backward_restated(p, x, gx, go)
    assert R.rel_l2(rec, g_eps) <= 1e-9
    xx = x.clone().requires_grad_(True)
    z1, ld = O.flow_forward(O.to_dtype(p, torch.float64), xx, torch.zeros(B, dtype=torch.float64))
    (back,) = torch.autograd.grad((z1 * g_eps).sum() + (ld * go).sum(), xx)
    assert R.rel_l2(back, gx) <= 1e-9
    # (2) implicit-function theorem
    via = R.params_via_forward(p, x, g_eps, go, torch.float64)
    assert sorted(via) == sorted(g_theta) and len(via) == 12 * O.depth_of(p)
    for k in via:
        assert R.rel_l2(via[k], g_theta[k]) <= 1e-9, k


def test_reverse_with_requires_grad_is_no_longer_refused_and_cpu_fails_loudly():
    net = lsnf_amd._netF(hps(4, depth=2), nz=8)
    eps = torch.zeros(3, 8, requires_grad=True)
    with pytest.raises(lsnf_amd.LsnfError):                     # not NotImplementedError: there is no CPU path, that is all
        net(eps, torch.zeros(3), reverse=True)
    with pytest.raises(lsnf_amd.LsnfError):
        net(torch.zeros(3, 8), torch.zeros(3, requires_grad=True), reverse=True, return_obj=True)
    with pytest.raises(lsnf_amd.LsnfError):
        lsnf_amd.flow.reverse_backward_z(None, torch.zeros(3, 8), None, torch.zeros(4))
    for prm in net.parameters():
        prm.requires_grad_(False)
    with pytest.raises(lsnf_amd.LsnfError):
        net(eps, torch.zeros(3), reverse=True)
