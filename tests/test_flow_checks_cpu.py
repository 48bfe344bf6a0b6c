"""CPU: every public wrapper of flow.py that takes tensors refuses well-shaped CPU tensors (and a plan built around CPU buffers)
with LsnfError before any entry point that launches is entered -- the argument checks are host-only Python and run without a GPU.
The wrapper names are listed explicitly: one added later and left out of WRAPPERS fails `test_every_tensor_wrapper_is_listed`."""
import inspect

import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)

import lsnf_amd
from counting_lib import QUERIES, install

F = lsnf_amd.flow
NZ, W, D, C, B = 8, 4, 2, 1, 5


class Ctx:
    def __init__(self):
        lib = lsnf_amd.load_library()
        self.plan = F.FlowPlan(NZ, W, D, C, torch.zeros(lib.lsnf_plan_floats(NZ, W, D, C)),
                               torch.zeros(lib.lsnf_prepare_scratch_bytes(NZ, W, D) // 8, dtype=torch.float64))
        self.params = [torch.zeros(s) for s in F._param_shapes(NZ, W, C) * D]
        self.z, self.v = torch.zeros(B, NZ), torch.zeros(B)
        self.saved = torch.zeros(D - 1, B, NZ)
        self.act = torch.zeros(max(lib.lsnf_act_saved_floats(NZ, W, D, B), 1))
        self.ws = torch.zeros(max(lib.lsnf_backward_params_workspace_floats(NZ, W, D, B), 4))
        self.state = torch.zeros(lib.lsnf_adam_state_bytes(NZ, W, D, C) // 4)
        self.rng = F.PhiloxNoise(3)


WRAPPERS = {
    "prepare": lambda c: F.prepare(c.params, NZ, W, D, C, plan=c.plan),
    "actnorm_init": lambda c: F.actnorm_init(c.params, c.z, NZ, W, D, C),
    "forward": lambda c: F.forward(c.plan, c.z, c.v, act_saved=c.act, z_saved_out=c.saved, params_ws=c.ws, stats=torch.zeros(264, dtype=torch.float64)),
    "BoundForward": lambda c: F.BoundForward(c.plan, c.z, (c.z.clone(), c.v.clone(), c.v.clone()))(None),
    "reverse": lambda c: F.reverse(c.plan, c.z, c.v, save_for_backward=True, act_saved=c.act),
    "backward_z": lambda c: F.backward_z(c.plan, c.z, c.saved, c.z, c.v, act_saved=c.act),
    "reverse_backward_z": lambda c: F.reverse_backward_z(c.plan, c.z, c.saved, c.act, c.z, c.v),
    "sample": lambda c: F.sample(c.plan, B, c.rng, want_eps=True, want_ll=True),
    "langevin_step": lambda c: F.langevin_step(c.plan, c.z, c.z, c.rng, 0.1),
    "reverse_langevin_step": lambda c: F.reverse_langevin_step(c.plan, c.z, c.saved, c.act, c.z, c.rng, 0.1),
    "backward_params": lambda c: F.backward_params(c.plan, c.params, c.z, c.z, c.saved, c.z, c.v, act_saved=c.act, workspace=c.ws),
    "adam_step": lambda c: F.adam_step(c.params, [torch.zeros_like(p) for p in c.params], c.state, NZ, W, D, C),
}


@pytest.mark.parametrize("name", ["prepare", "actnorm_init", "forward", "BoundForward", "reverse", "backward_z", "reverse_backward_z",
                                  "sample", "langevin_step", "reverse_langevin_step", "backward_params", "adam_step"])
def test_cpu_tensors_are_refused_before_any_launch(name, monkeypatch):
    stand = install(monkeypatch, lsnf_amd)
    with pytest.raises(lsnf_amd.LsnfError):
        WRAPPERS[name](Ctx())
    assert stand.launching() == [], (name, dict(stand.entered))


def test_every_tensor_wrapper_is_listed():
    """A public function of flow.py with a tensor (or plan, or parameter-list) argument is one of WRAPPERS, or is named here as
    one that launches nothing."""
    no_launch = {"params_from_state_dict", "new_act_saved", "new_params_workspace", "reverse_keep_supported", "adam_state_views",
                 "block_prefix", "alloc_plan", "new_stats", "new_adam_state"}
    takes = ("Tensor", "FlowPlan")
    public = {n for n, f in vars(F).items() if inspect.isfunction(f) and f.__module__ == F.__name__ and not n.startswith("_")
              and any(t in str(p.annotation) for p in inspect.signature(f).parameters.values() for t in takes)}
    assert public - no_launch == set(WRAPPERS) - {"BoundForward"}
    assert inspect.isclass(F.BoundForward)


def test_the_stand_in_counts_and_passes_through(monkeypatch):
    stand = install(monkeypatch, lsnf_amd)
    assert F.adam_state_bytes(NZ, W, D, C) == lsnf_amd.load_library().lsnf_adam_state_bytes(NZ, W, D, C) > 0
    assert stand.entered["lsnf_adam_state_bytes"] == 1 and stand.launching() == []
    rc = stand.lsnf_forward(None, NZ, W, D, C, 0, D, B, *([None] * 10))          # a NULL plan: refused by the library's own validation, no HIP call
    assert rc != 0 and stand.launching() == ["lsnf_forward"]
    assert QUERIES < set(lsnf_amd.exported_symbols())
