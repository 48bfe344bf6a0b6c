"""The case table of tests/test_gpu_shape_forms.py (tests/shape_forms_worker.py), on the CPU: every documented value of every
workgroup-shape knob is in the environment of at least one child, so that a later edit cannot drop one silently."""
import csv
import os
import re

import shape_forms_worker as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_knob_value_is_in_some_childs_environment():
    for knob, values in W.KNOB_VALUES.items():
        for v in values:
            assert any(env.get(knob) == v for _, env in W.CHILDREN), (knob, v)
    assert W.CHILDREN[0] == ("baseline", {}) and len(W.CHILDREN) <= 8
    assert len({name for name, _ in W.CHILDREN}) == len(W.CHILDREN)
    for _, env in W.CHILDREN:                   # a child sets documented knobs only, and runs the groups they address
        assert set(env) <= set(W.KNOB_VALUES)
        assert W.groups_of(env)
    assert set(W.groups_of({})) == set(W.GROUP_KNOBS)


def test_the_knobs_are_those_integration_md_documents():
    """INTEGRATION.md section 4 lists the knobs that choose among kernel instantiations: the table covers each of them but the two
    that have setters (LSNF_MATH, LSNF_SMALL_MAX: the `kernels` fixture of conftest.py drives those in every kernel-level test)."""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    documented = set(re.findall(r"^\| `(LSNF_[A-Z0-9_]+)` \|.*every value computes the same documented result", text, re.M))
    assert documented - {"LSNF_MATH", "LSNF_SMALL_MAX"} == set(W.KNOB_VALUES)


def test_rows_per_workgroup_follow_the_knob_value():
    assert W.edge_rows(64) == [1, 17, 63, 64, 65, 161]
    assert [W.fwd3q_rows({"LSNF_FWD3Q_SHAPE": c}) for c in ("41", "81", "42", "82", "242")] == [(64, 128), (128, 128), (128, 128), (256, 256), (128, 128)]
    assert W.fwd3q_rows({}) == (64, 128) and W.waves_rows({}) == (128, 128)
    assert W.waves_rows({"LSNF_FORCE_WAVES": "8", "LSNF_FWD_WAVES": "4"}) == (256, 128)
    assert W.small3_st({"LSNF_SMALL3_ST": "4"}, "C3") == (4, 4) and W.small3_st({"LSNF_SMALL3_ST": "4"}, "C5") == (4, 2)
    assert 2 * 256 + 33 <= W.N_SMALL
    small, lds, x3 = W.tn_rows({"LSNF_TN_CHUNK": "16"})
    assert small == [1, 15, 16, 17, 65] and [B % 16 for B in lds + x3] == [0, 1, 1, 0, 1, 15]
    assert [B % 4096 for B in W.tn_rows({"LSNF_TN_CHUNK": "4096"})[1]] == [0, 1, 17]


def test_the_mala_probes_meet_a_ragged_half_and_an_empty_half_tile():
    """The forced LSNF_SMALL3_ST forms of the two MALA kernels run entries of tests/chain_geometries.py too: a ragged half and a
    second half-tile that is entirely padding, under every ST (both are <2, 2>, which has all three), at the batch sizes of the
    other MALA probes.  They are not in GEOS: its sorted order seeds the inputs of every other probe."""
    import chain_geometries as G
    assert not set(W.CHAIN_GEOS) & set(W.GEOS) and set(W.MALA_GEOS) == {"C3", "C5", "tiny"} | set(W.CHAIN_GEOS)
    geos = set(W.CHAIN_GEOS.values())
    assert geos <= set(G.GEOS) and all(G.pick_tiles(nz // 2, w) == (2, 2) for nz, w, _, _ in geos)
    assert any(G.draw_straddles(g) and not G.second_half_tile_empty(g) for g in geos) and any(G.second_half_tile_empty(g) for g in geos)
    for name in W.MALA_GEOS:
        assert W.geo_of(name) == (W.GEOS[name] if name in W.GEOS else W.CHAIN_GEOS[name])
    sts = set()
    for name in W.CHAIN_GEOS:
        for _, env in W.CHILDREN:
            if "small3" in W.groups_of(env):
                want, runs = W.small3_st(env, name)
                assert want == runs and {1, 17, 97} <= set(W.mala_rows(env, name))
                sts.add(runs)
    assert sts == {1, 2, 4}


def test_the_latency_shapes_of_the_table_are_those_the_recorded_run_launched():
    """small3_st restates the give-way rule of lsnf_small3_*_st (a shape that is not built, or whose LDS does not fit, gives way to
    the next smaller one).  profiles/shape_forms_kernel_calls.csv is what the module's children really launched: per latency kernel
    and tile geometry, the ST values in it are exactly those the table says its geometries ran."""
    ran = {}
    for geo, (nz, width, _, _) in W.GEOS.items():
        cfg = (1, 1) if nz <= 64 and width <= 32 else (2, 2) if width <= 64 else (2, 4)        # csrc: lsnf_pick_tiles
        for _, env in W.CHILDREN:
            if "small3" in W.groups_of(env):
                ran.setdefault(cfg, set()).add(W.small3_st(env, geo)[1])
    assert ran == {(1, 1): {1, 2, 4}, (2, 2): {1, 2, 4}, (2, 4): {1, 2}}
    seen = {}
    with open(os.path.join(ROOT, "profiles", "shape_forms_kernel_calls.csv"), newline="") as f:
        for row in csv.DictReader(f):
            m = re.match(r"(lsnf_small3_(?:fwd|rev|bwd|rbwd|mala|rmala)_kernel)<(\d), (\d), (\d)[,>]", row["kernel"])
            if m and int(row["calls"]) > 0:
                seen.setdefault((m.group(1), (int(m.group(2)), int(m.group(3)))), set()).add(int(m.group(4)))
    assert len(seen) == 6 * 3
    for (kernel, cfg), sts in seen.items():
        assert sts == ran[cfg], (kernel, cfg, sts)
