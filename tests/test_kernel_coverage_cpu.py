"""tools/kernel_coverage.py on a hand-written kernel-stats table and a stub list of built instantiations (no GPU, no build): the
demangled names of a trace are brought to the short form of tools/kernel_resources.py, calls of several files add up, and the
three lists -- launched, never launched, unmatched -- are what the table says."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_coverage as KC  # noqa: E402
import kernel_resources as KR  # noqa: E402

AN = "(anonymous namespace)::"
NAMES = [
    (f"void {AN}lsnf_rev_kernel<{AN}RevCfg<1, 1>, 8, true>({AN}RevArgs)", "lsnf_rev_kernel<1, 1, 8, true>"),
    (f"void {AN}lsnf_small3_rev_kernel<{AN}Small3RevCfg<2, 4>, 2, false, true>({AN}Small3RevArgs)", "lsnf_small3_rev_kernel<2, 4, 2, false, true>"),
    (f"void {AN}lsnf_bwd3_kernel<{AN}Bwd3Cfg<2, 4>, 8, 2>({AN}Bwd3Args)", "lsnf_bwd3_kernel<2, 4, 8, 2>"),
    (f"void {AN}lsnf_fwd3q_kernel<2, 4, 2, 0, 1>({AN}Fwd3pArgs)", "lsnf_fwd3q_kernel<2, 4, 2, 0, 1>"),
    (f"void {AN}lsnf_small_fwd_kernel<{AN}SmallFwdCfg<2, 4> >({AN}SmallFwdArgs)", "lsnf_small_fwd_kernel<2, 4>"),
    (f"void {AN}lsnf_tn_gemm_lds_kernel<4, false>({AN}TnArgs)", "lsnf_tn_gemm_lds_kernel<4, false>"),
    (f"void {AN}lsnf_contract_x3_kernel<true>({AN}X3Args)", "lsnf_contract_x3_kernel<true>"),
    (f"void {AN}lsnf_adam_kernel<(bool)1, (bool)0, false>({AN}AdamArgs).kd","lsnf_adam_kernel<true, false, false>"),
    ("void lsnf_gj_kernel<32>(LsnfParamPtrs, int, double*)", "lsnf_gj_kernel<32>"),
    ("lsnf_pack_kernel(LsnfParamPtrs, LsnfGeo, double const*, float*)", "lsnf_pack_kernel"),
    (f"{AN}lsnf_unfold_kernel(LsnfParamPtrs, LsnfGradPtrs, float const*, double const*, float const*, int, int, int)", "lsnf_unfold_kernel"),
    ("void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<double>, std::array<char*, 1ul> >(int, at::native::FillFunctor<double>, std::array<char*, 1ul>)",
     "void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<double>, std::array<char*, 1ul> >(int, at::native::FillFunctor<double>, std::array<char*, 1ul>)"),
    ("__amd_rocclr_copyBuffer", "__amd_rocclr_copyBuffer"),
]


@pytest.mark.parametrize("demangled,short", NAMES, ids=[s[:40] for _, s in NAMES])
def test_short_name_of_a_demangled_name(demangled, short):
    assert KC.short_name(demangled) == short


def test_short_names_agree_with_the_mangled_form():
    """The same instantiation through both parsers: the code objects' mangled name (kernel_resources._short) and the trace's."""
    pairs = [("_ZN12_GLOBAL__N_115lsnf_rev_kernelINS_6RevCfgILi1ELi1EEELi8ELb1EEEvNS_7RevArgsE",
              f"void {AN}lsnf_rev_kernel<{AN}RevCfg<1, 1>, 8, true>({AN}RevArgs)"),
             ("_ZN12_GLOBAL__N_122lsnf_small3_rev_kernelINS_12Small3RevCfgILi2ELi4EEELi2ELb0ELb1EEEvNS_13Small3RevArgsE",
              f"void {AN}lsnf_small3_rev_kernel<{AN}Small3RevCfg<2, 4>, 2, false, true>({AN}Small3RevArgs)"),
             ("_ZN12_GLOBAL__N_117lsnf_fwd3q_kernelILi2ELi4ELi2ELi0ELi1EEEvNS_9Fwd3pArgsE", f"void {AN}lsnf_fwd3q_kernel<2, 4, 2, 0, 1>({AN}Fwd3pArgs)"),
             ("_Z14lsnf_gj_kernelILi32EEv13LsnfParamPtrsiPd", "void lsnf_gj_kernel<32>(LsnfParamPtrs, int, double*)"),
             ("_Z16lsnf_pack_kernel13LsnfParamPtrs7LsnfGeoPKdPf", "lsnf_pack_kernel(LsnfParamPtrs, LsnfGeo, double const*, float*)")]
    for mangled, demangled in pairs:
        assert KR._short(mangled) == KC.short_name(demangled)


BUILT = ["lsnf_rev_kernel<1, 1, 8, true>", "lsnf_rev_kernel<1, 1, 8, false>", "lsnf_bwd3_kernel<2, 4, 8, 2>", "lsnf_bwd3_kernel<2, 4, 4, 2>",
         "lsnf_fwd3q_kernel<2, 4, 2, 0, 0>", "lsnf_fwd3q_kernel<2, 4, 2, 0, 1>", "lsnf_tn_gemm_lds_kernel<4, false>",
         "lsnf_tn_gemm_lds_kernel<4, true>", "lsnf_pack_kernel", "lsnf_gj_kernel<32>"]
STATS_A = f'''"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"
"void {AN}lsnf_rev_kernel<{AN}RevCfg<1, 1>, 8, true>({AN}RevArgs)",3,300,100.0,10.0,90,110,1.0
"void {AN}lsnf_bwd3_kernel<{AN}Bwd3Cfg<2, 4>, 8, 2>({AN}Bwd3Args)",2,200,100.0,10.0,90,110,1.0
"void {AN}lsnf_fwd3q_kernel<2, 4, 2, 0, 1>({AN}Fwd3pArgs)",1903,414819312,217981.77,99.90,97441,1003440,92339.6
"lsnf_pack_kernel(LsnfParamPtrs, LsnfGeo, double const*, float*)",1,40400,40400.0,9.7e-03,40400,40400,0.0
"__amd_rocclr_copyBuffer",50,144281,2885.62,0.0347,2201,7040,1004.7
"void at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<double>, std::array<char*, 1ul> >(int, at::native::FillFunctor<double>, std::array<char*, 1ul>)",9,28160,3128.8,6.7e-03,1360,5120,1719.0
'''
STATS_B = f'''kernel,calls
"void {AN}lsnf_rev_kernel<{AN}RevCfg<1, 1>, 8, true>({AN}RevArgs)",4
"void {AN}lsnf_tn_gemm_lds_kernel<4, false>({AN}TnArgs)",5
"void lsnf_gj_kernel<32>(LsnfParamPtrs, int, double*)",1
'''


def _write(tmp_path, **files):
    paths = []
    for name, text in files.items():
        (tmp_path / name).write_text(text)
        paths.append(str(tmp_path / name))
    return paths


def test_three_lists(tmp_path):
    calls = KC.read_calls(_write(tmp_path, a_kernel_stats=STATS_A, b_kernel_calls=STATS_B))
    launched, never, unmatched = KC.ledger(BUILT, calls)
    assert launched == {"lsnf_rev_kernel<1, 1, 8, true>": 7, "lsnf_bwd3_kernel<2, 4, 8, 2>": 2, "lsnf_fwd3q_kernel<2, 4, 2, 0, 1>": 1903,
                        "lsnf_pack_kernel": 1, "lsnf_tn_gemm_lds_kernel<4, false>": 5, "lsnf_gj_kernel<32>": 1}
    assert never == ["lsnf_bwd3_kernel<2, 4, 4, 2>", "lsnf_fwd3q_kernel<2, 4, 2, 0, 0>", "lsnf_rev_kernel<1, 1, 8, false>",
                     "lsnf_tn_gemm_lds_kernel<4, true>"]
    assert unmatched == {}                                   # the framework's kernels are not the library's: not listed
    text = KC.render(launched, never, unmatched, 2)
    assert "10 built instantiations, 6 launched, 4 never launched" in text and "      1903  lsnf_fwd3q_kernel<2, 4, 2, 0, 1>" in text


def test_a_name_of_another_build_is_reported(tmp_path):
    """A kernel of the library that the build does not have (here: an instantiation without its last template argument, as a trace
    of an older build names it) lands in the third list -- and nowhere else."""
    stats = f'kernel,calls\n"void {AN}lsnf_fwd3q_kernel<2, 4, 2, 1>({AN}Fwd3pArgs)",4\n'
    launched, never, unmatched = KC.ledger(BUILT, KC.read_calls(_write(tmp_path, old=stats)))
    assert launched == {} and len(never) == len(BUILT) and unmatched == {"lsnf_fwd3q_kernel<2, 4, 2, 1>": 4}


def test_command_line(tmp_path, monkeypatch, capsys):
    """main(): the built names come from kernel_resources.collect (stubbed: no objects here), exit status 1 iff a name is unmatched."""
    monkeypatch.setattr(KR, "collect", lambda build_dir, match: {n: {} for n in BUILT})
    paths = _write(tmp_path, a_kernel_stats=STATS_A, b_kernel_calls=STATS_B)
    out_csv = tmp_path / "calls.csv"
    monkeypatch.setattr(sys, "argv", ["kernel_coverage.py", "BUILD"] + paths + ["--calls-csv", str(out_csv)])
    assert KC.main() == 0
    assert "never launched (4):" in capsys.readouterr().out
    rows = out_csv.read_text().splitlines()
    assert rows[0] == "kernel,calls" and '"lsnf_rev_kernel<1, 1, 8, true>",7' in rows and not any("rocclr" in r or "at::" in r for r in rows)
    bad = _write(tmp_path, old=f'kernel,calls\n"void {AN}lsnf_fwd3q_kernel<2, 4, 2, 1>({AN}Fwd3pArgs)",4\n')
    monkeypatch.setattr(sys, "argv", ["kernel_coverage.py", "BUILD"] + bad)
    assert KC.main() == 1
