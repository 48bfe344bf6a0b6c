"""CPU: the deterministic parameter gradients without a GPU -- `lsnf_backward_params_det` and its size query are declared,
exported and bound (ABI still 5), the workspace is the default one plus a partials area whose size follows from the documented
chunk count alone, the entry point validates its arguments before any HIP call, and the Python layers carry the opt-in
(`deterministic=False` keywords, `_netF.deterministic_grads = False`).  None of this holds without the feature."""
import ctypes
import inspect
import os
import re
import types

import pytest

from conftest import ROOT

import lsnf_amd

LSNF_OK, LSNF_E_ARG, LSNF_E_GEOMETRY = 0, -1, -2
SYMBOLS = ("lsnf_backward_params_det_workspace_floats", "lsnf_backward_params_det")
X3_MIN_ROWS, MAX_CHUNKS = 12288, 128          # csrc/lsnf_layout.h LSNF_X3_MIN_ROWS, LSNF_DET_MAX_CHUNKS


def test_symbols_are_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lsnf_flow.h")).read(), flags=re.S)
    lib = lsnf_amd.load_library()
    for name in SYMBOLS:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, hdr), name
        assert hasattr(lib, name)
        assert name in lsnf_amd._lib._SIGNATURES and name in lsnf_amd.exported_symbols()
    assert lsnf_amd._lib._SIGNATURES["lsnf_backward_params_det"] == lsnf_amd._lib._SIGNATURES["lsnf_backward_params"]
    assert lib.lsnf_abi_version() == 5                          # symbols were added, nothing else changed


def fold_floats(nz, w):
    """LsnfFoldLayout.per_block: the folded gradients of one block, rounded up to 4 floats."""
    half = nz // 2
    return (nz * nz + nz + half * w + w + w * w + w + 2 * (w * half + half) + 3) // 4 * 4


def chunks(B, depth):
    """The documented chunk count the workspace holds slots for (include/lsnf_flow.h, csrc/lsnf_layout.h)."""
    rows = 512 if B >= 16384 else 128
    if -(-B // rows) > MAX_CHUNKS:
        rows = (-(-B // MAX_CHUNKS) + 15) // 16 * 16
    fp32 = -(-B // rows)
    x3 = 0
    if B >= X3_MIN_ROWS:
        rows3 = (-(-B // max(256 // depth, 1)) + 31) // 32 * 32
        x3 = -(-B // rows3)
    return max(fp32, x3)


@pytest.mark.parametrize("nz,w,depth", [(128, 64, 5), (100, 128, 5), (50, 33, 5), (128, 64, 1), (8, 4, 16)])
def test_workspace_is_the_default_one_plus_the_partials(nz, w, depth):
    lib = lsnf_amd.load_library()
    plain = lambda B: lib.lsnf_backward_params_workspace_floats(nz, w, depth, B)
    det = lambda B: lib.lsnf_backward_params_det_workspace_floats(nz, w, depth, B)
    for B in (1, 100, 128, 129, 1500, 5000, 12288, 16383, 16384, 65536, 65537, 100000, 1 << 20):
        assert det(B) >= plain(B) > 0
        assert det(B) % 4 == 0
        # the difference depends on B only through the chunk count: chunks x one image of the whole fold
        assert det(B) - (plain(B) + 3) // 4 * 4 == chunks(B, depth) * depth * fold_floats(nz, w), B
    assert chunks(100, depth) == 1 and chunks(8192, 5) == 64 and chunks(65536, 5) == 128 and chunks(1 << 20, 5) <= MAX_CHUNKS
    assert det(0) == (plain(0) + 3) // 4 * 4
    assert lib.lsnf_backward_params_det_workspace_floats(130, w, depth, 100) == 0
    assert lib.lsnf_backward_params_det_workspace_floats(nz, w, 17, 100) == 0
    assert lib.lsnf_backward_params_det_workspace_floats(nz, w, depth, -1) == 0


def test_documented_size_at_the_headline_shape():
    """include/lsnf_flow.h: 663 040 bytes per chunk at nz 128 / width 64 / depth 5, 128 chunks at 65 536 rows."""
    lib = lsnf_amd.load_library()
    extra = lib.lsnf_backward_params_det_workspace_floats(128, 64, 5, 65536) - lib.lsnf_backward_params_workspace_floats(128, 64, 5, 65536)
    assert extra * 4 == 128 * 663040


def _named(lib, name):
    return name.encode() in lib.lsnf_last_error()


def test_det_entry_validates_before_any_hip_call():
    lib = lsnf_amd.load_library()
    nz, w, d = 128, 64, 5
    fake = [0x10000 * (i + 1) for i in range(8)]          # 16-byte aligned addresses that are never dereferenced on the host
    plan, z_in, z_out, saved, ws = fake[:5]
    tab = (ctypes.c_void_p * (d * 12))(*[0x900000 + 64 * i for i in range(d * 12)])

    def call(nz=nz, w=w, d=d, c=1, B=4, plan=plan, params=tab, grads=tab, z_in=z_in, z_out=z_out, saved=saved, act=None, g_z1=None,
             g_logdet=None, g_in=None, ws=ws):
        return lib.lsnf_backward_params_det(plan, params, grads, nz, w, d, c, B, z_in, z_out, saved, act, g_z1, g_logdet, 1, -0.25,
                                            g_in, ws, None)

    assert call(nz=130) == LSNF_E_GEOMETRY and call(d=17) == LSNF_E_GEOMETRY
    for kw in (dict(B=0), dict(B=-3), dict(plan=None), dict(params=None), dict(grads=None), dict(z_in=None), dict(z_out=None),
               dict(saved=None), dict(ws=None),
               dict(plan=plan + 4), dict(ws=ws + 8), dict(z_in=z_in + 2), dict(z_out=z_out + 1), dict(saved=saved + 3),
               dict(g_z1=fake[5] + 2), dict(g_logdet=fake[5] + 1), dict(g_in=fake[6] + 2), dict(act=fake[7] + 4)):
        assert call(**kw) == LSNF_E_ARG, kw
        assert _named(lib, "lsnf_backward_params_det"), (kw, lib.lsnf_last_error())
    bad = (ctypes.c_void_p * (d * 12))(*[0x900000 + 64 * i for i in range(d * 12)])
    bad[7] = None
    assert call(params=bad) == LSNF_E_ARG and b"pointer 7" in lib.lsnf_last_error()
    bad[7] = 0x900002
    assert call(grads=bad) == LSNF_E_ARG and b"pointer 7" in lib.lsnf_last_error()
    # the default entry point still names itself
    assert lib.lsnf_backward_params(None, tab, tab, nz, w, d, 1, 4, z_in, z_out, saved, None, None, None, 1, -0.25, None, ws, None) == LSNF_E_ARG
    assert b"lsnf_backward_params:" in lib.lsnf_last_error()


def test_python_layers_carry_the_opt_in():
    F = lsnf_amd.flow
    for fn in (F.backward_params, F.new_params_workspace):
        p = inspect.signature(fn).parameters["deterministic"]
        assert p.default is False
    assert inspect.signature(F.backward_params).parameters["deterministic"].kind is inspect.Parameter.KEYWORD_ONLY
    hps = types.SimpleNamespace(f_n_levels=1, f_depth=2, f_flow_permutation=2, f_width=4, f_flow_coupling=1)
    net = lsnf_amd._netF(hps, nz=8)
    assert net.deterministic_grads is False and net.reverse_keeps_stash is False
    net.deterministic_grads = True
    assert "deterministic_grads" not in net.state_dict() and len(net.state_dict()) == 2 * 17


def test_default_path_never_enters_the_det_size_query(monkeypatch):
    """The default `new_params_workspace` / `backward_params` ask the existing size query only; the new one is entered with
    deterministic=True alone (and a CPU workspace is then refused before any launching entry point)."""
    import torch
    from counting_lib import install
    F = lsnf_amd.flow
    lib = lsnf_amd.load_library()
    NZ, W, D, B = 8, 4, 2, 7                  # (a batch size no other test of the process has cached a size for)
    plan = F.FlowPlan(NZ, W, D, 1, torch.zeros(lib.lsnf_plan_floats(NZ, W, D, 1)), torch.zeros(8, dtype=torch.float64))
    stand = install(monkeypatch, lsnf_amd)
    n_plain = F.new_params_workspace(plan, B, "cpu").numel()
    assert "lsnf_backward_params_det_workspace_floats" not in stand.entered
    n_det = F.new_params_workspace(plan, B, "cpu", deterministic=True).numel()
    assert stand.entered["lsnf_backward_params_det_workspace_floats"] == 1
    assert n_det == lib.lsnf_backward_params_det_workspace_floats(NZ, W, D, B) > n_plain
    params = [torch.zeros(s) for s in F._param_shapes(NZ, W, 1) * D]
    z, saved = torch.zeros(B, NZ), torch.zeros(D - 1, B, NZ)
    with pytest.raises(lsnf_amd.LsnfError):
        F.backward_params(plan, params, z, z, saved, ll_scale=-1.0, deterministic=True)
    assert set(stand.launching()) <= {"lsnf_backward_params_det_workspace_floats"}       # (a size query: it launches nothing)
