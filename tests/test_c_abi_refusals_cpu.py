"""CPU: every refusal of the C ABI, with its code, its full message and its precedence over every other single violation of the
same call, is what tests/golden/c_abi_refusals.json holds (recorded by tests/golden/make_c_abi_refusals.py, which also defines the
matrix).  The calls are issued from one fresh child process that sees no device, and no case may be anything but a refusal
or an empty batch: a rule that got lost shows as LSNF_E_HIP there, never as a launch on the made-up addresses."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN_DIR

import lsnf_amd
from counting_lib import QUERIES

spec = importlib.util.spec_from_file_location("make_c_abi_refusals", os.path.join(GOLDEN_DIR, "make_c_abi_refusals.py"))
M = importlib.util.module_from_spec(spec)
spec.loader.exec_module(M)

# size queries that postdate counting_lib's list: they launch nothing either
SIZE_QUERIES = {"lsnf_adam_state_bytes_ex", "lsnf_backward_params_det_workspace_floats"}


@pytest.fixture(scope="module")
def recorded():
    with open(M.FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def answered():
    return M.answers(lsnf_amd._lib.LIB_PATH)      # asserts that no case passed validation


def test_matrix_covers_every_entry_point_that_can_launch(recorded):
    launching = set(lsnf_amd.exported_symbols()) - QUERIES - SIZE_QUERIES
    assert "lsnf_adam_step_ex" in launching
    assert {M.entry_point(name) for name in M.ENTRIES} == launching
    assert list(recorded["entries"]) == list(M.ENTRIES)
    for name, rec in recorded["entries"].items():
        assert rec["violations"] == [v[0] for v in M.violations(name)]
        n = len(rec["violations"])
        assert len(M.cases(name)) == n * n == len(rec["answer"]) == len(rec["empty_batch"])      # singles and all ordered pairs


def test_no_recorded_case_can_reach_a_launch(recorded):
    for name, rec in recorded["entries"].items():
        for k, empty in zip(rec["answer"], rec["empty_batch"]):
            code, message = recorded["answers"][k]
            assert M.cannot_launch(code, 0 if empty else 1), (name, code, message)
            assert (code == M.LSNF_OK) == (message == "")


def test_library_answers_as_recorded(recorded, answered):
    wrong = []
    for name, rec in recorded["entries"].items():
        names = rec["violations"]
        for (i, j), k, (code, message, _) in zip(M.cases(name), rec["answer"], answered[name]):
            if [code, message] != recorded["answers"][k]:
                wrong.append("%s [%s; %s]: %r, recorded %r" % (name, names[i], names[j], [code, message], recorded["answers"][k]))
    assert not wrong, "%d cases differ, the first: %s" % (len(wrong), "\n".join(wrong[:10]))


def test_recorder_reproduces_the_fixture(answered):
    with open(M.FIXTURE) as f:
        assert M.dumps(M.encode(answered)) == f.read()
