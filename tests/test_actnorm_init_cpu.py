"""CPU: the data-dependent actnorm init's C ABI surface (symbols, workspace query) and the fp64 restatement the GPU tests
use at large batch sizes, pinned to the reference's fixtures (tests/golden/init/, tests/golden/make_golden_init.py)."""
import pytest
import torch

import lsnf_amd
from init_restated import bounds, init_error, init_names, load_init, restated_init, written_keys


def test_init_symbols_are_exported():
    lib = lsnf_amd.load_library()
    for name in ("lsnf_actnorm_init", "lsnf_actnorm_init_workspace_bytes"):
        assert hasattr(lib, name)
        assert name in lsnf_amd.exported_symbols()


def test_init_workspace_query_needs_no_gpu():
    q = lsnf_amd.flow.actnorm_init_workspace_bytes
    for nz, w, d, c in ((128, 64, 5, 1), (100, 128, 5, 1), (2, 1, 1, 1), (20, 12, 5, 0), (126, 127, 16, 0)):
        assert q(nz, w, d, c, 1) > 0
    for nz, w, d, c, B in ((130, 64, 5, 1, 100), (7, 4, 5, 1, 100), (128, 129, 5, 1, 100), (128, 64, 17, 1, 100),
                           (128, 64, 5, 1, 0), (128, 64, 0, 1, 100), (128, 64, 5, 2, 100), (0, 4, 5, 1, 10)):
        assert q(nz, w, d, c, B) == 0, (nz, w, d, c, B)
    sizes = [q(128, 64, 5, 1, B) for B in (1, 2, 255, 256, 257, 1000, 65536)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert q(128, 64, 5, 1, 65536) >= 65536 * (2 * 128 + 2 * 64) * 4      # block I/O ping-pong + two pre-activations


def test_init_rejects_cpu_tensors_before_launch():
    nz, w, d = 8, 4, 1
    params = [torch.zeros(s) for s in lsnf_amd.flow._param_shapes(nz, w, 1)]
    with pytest.raises(lsnf_amd.LsnfError):
        lsnf_amd.flow.actnorm_init(params, torch.zeros(3, nz), nz, w, d, 1)
    with pytest.raises(lsnf_amd.LsnfError, match="unsupported geometry"):
        lsnf_amd.flow.actnorm_init(params, torch.zeros(3, 9), 9, w, d, 1)


@pytest.mark.parametrize("name", init_names())
def test_restated_init_reproduces_reference_fixture(name):
    p, ref32, ref64, g = load_init(name)
    depth = int(g["meta_depth"])
    q, rms = restated_init(p, torch.from_numpy(g["z"]), int(g["meta_coupling"]))
    tol_logs, tol_b = bounds(ref32, ref64, rms, depth)
    e_logs, e_b = init_error(q, ref32, rms, depth)
    assert e_logs <= tol_logs and e_b <= tol_b, (e_logs, e_b)
    e_logs, e_b = init_error(q, ref64, rms, depth)            # the restatement IS the reference's init in fp64
    assert e_logs <= 1e-12 and e_b <= 1e-12, (e_logs, e_b)
    for k in written_keys(depth):                             # the fixture does show the init: every written tensor moved
        assert not torch.equal(p[k].double(), torch.from_numpy(ref32[k]).double()), k
    if int(g["meta_B"]) == 1:                                 # var = 0: logs = log(1 / 1e-6) / 3, b = -x
        for k in written_keys(depth):
            if k.endswith("logs"):
                assert abs(float(ref32[k].max()) - torch.log(torch.tensor(1e6, dtype=torch.float64)).item() / 3) <= 1e-6
