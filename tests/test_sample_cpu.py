"""CPU: fused prior sampling without a GPU -- `lsnf_sample` is declared / exported / bound and validates its arguments before
any HIP call; the module's `sample` fails loudly on the CPU; and the definition of `ll_out` is pinned on the float64 oracle
(that last check holds with or without the feature; the others need it)."""
import ctypes
import math
import os
import re
import types

import pytest
import torch

from conftest import ROOT
from oracle import flow_oracle as O
import sample_restated as S

import lsnf_amd

LSNF_OK, LSNF_E_ARG, LSNF_E_GEOMETRY = 0, -1, -2


def test_symbol_is_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+lsnf_sample\s*\(", hdr)
    lib = lsnf_amd.load_library()
    assert hasattr(lib, "lsnf_sample")
    assert "lsnf_sample" in lsnf_amd._lib._SIGNATURES and "lsnf_sample" in lsnf_amd.exported_symbols()
    assert lib.lsnf_abi_version() == 5                          # a symbol was added, nothing else changed
    assert callable(lsnf_amd.flow.sample) and callable(lsnf_amd.langevin.sample_x)


def test_argument_validation_runs_before_any_hip_call():
    lib = lsnf_amd.load_library()
    Rng = lsnf_amd._lib.LsnfRng

    def call(nz, w, d, c, B, rng=Rng(1, 0, None, 0), T=1.0, z_out=None, eps_out=None):
        return lib.lsnf_sample(None, nz, w, d, c, B, None if rng is None else ctypes.byref(rng), T, z_out, None, eps_out, None, None)

    assert call(130, 64, 5, 1, 4) == LSNF_E_GEOMETRY and call(128, 64, 17, 1, 4) == LSNF_E_GEOMETRY
    assert call(128, 64, 5, 1, -1) == LSNF_E_ARG
    assert b"lsnf_sample" in lib.lsnf_last_error()
    assert call(128, 64, 5, 1, 0) == LSNF_OK                    # empty batch: nothing to launch, NULL pointers allowed
    assert call(2, 1, 1, 0, 0) == LSNF_OK and call(126, 127, 16, 1, 0) == LSNF_OK
    assert call(128, 64, 5, 1, 4) == LSNF_E_ARG                 # NULL plan / z_out
    for B in (0, 4):                                            # the generator's rules hold for an empty batch too
        assert call(128, 64, 5, 1, B, rng=None) == LSNF_E_ARG and b"rng" in lib.lsnf_last_error()
        assert call(128, 64, 5, 1, B, rng=Rng(1, 0, None, -1)) == LSNF_E_ARG and b"row0" in lib.lsnf_last_error()
        assert call(128, 64, 5, 1, B, rng=Rng(1, 0, 12, 0)) == LSNF_E_ARG and b"offset_dev" in lib.lsnf_last_error()
        for T in (-0.5, float("nan"), float("inf"), -float("inf")):
            assert call(128, 64, 5, 1, B, T=T) == LSNF_E_ARG and b"temperature" in lib.lsnf_last_error()
    assert call(128, 64, 5, 1, 0, T=0.0) == LSNF_OK


def test_module_sample_has_no_cpu_path():
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=8, f_flow_coupling=1)
    net = lsnf_amd._netF(hps, nz=8)
    with pytest.raises(lsnf_amd.LsnfError):
        net.sample(4, lsnf_amd.flow.PhiloxNoise(1))
    with pytest.raises(lsnf_amd.LsnfError):
        with torch.no_grad():
            net.sample(4, 7, return_log_prob=True)


@pytest.mark.parametrize("nz,w,depth,coupling", [(8, 4, 5, 1), (20, 12, 3, 0), (126, 127, 2, 1)])
def test_ll_is_the_forward_log_prob_at_x(nz, w, depth, coupling):
    """ll(eps, obj) = oracle.log_prob(eps, -obj), and the forward at x = flow_reverse(eps) returns (eps, -obj): the ll_out of
    lsnf_sample is the ll_out lsnf_forward documents, evaluated at the sample."""
    p = O.init_params(nz, w, depth, seed=5)
    if coupling == 0:
        for i in range(depth):
            for k in ("f.fc_zeros.w", "f.fc_zeros.b", "f.fc_zeros.logs"):
                p[O.block_prefix(i) + k] = p[O.block_prefix(i) + k][:, : nz // 2].contiguous()
    for T in (1.0, 0.7, 0.0):
        eps, x, obj, ll = S.sample(p, 33, nz, seed=2 ** 63 + 5, offset=(1 << 40) + 3, row0=2 ** 32 - 5, temperature=T)
        assert eps.dtype == torch.float64 and eps.shape == (33, nz) and bool(torch.isfinite(eps).all())
        assert (ll - O.log_prob(eps, -obj)).abs().max().item() <= 1e-9
        z1, logdet, ll_fwd = O.flow_log_prob(O.to_dtype(p, torch.float64), x, coupling)
        scale = max(1.0, ll.abs().max().item())
        assert (z1 - eps).abs().max().item() <= 1e-9 and (logdet + obj).abs().max().item() <= 1e-9 * scale
        assert (ll_fwd - ll).abs().max().item() <= 1e-9 * scale
    assert abs(S.ll(torch.zeros(1, nz, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)).item() - math.log(2 * math.pi)) < 1e-15
