"""ctypes binding of liblsnf_flow.so (C ABI: include/lsnf_flow.h).

The library is the product; there is no fallback.  If the shared object is missing or a
symbol is absent, import of the compute API raises -- nothing is silently routed elsewhere."""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# LSNF_LIB_PATH: developer override to A/B alternative BUILDS of the same library (tools/); not a fallback.
LIB_PATH = os.environ.get("LSNF_LIB_PATH") or os.path.join(_HERE, "liblsnf_flow.so")

LSNF_PARAMS_PER_BLOCK = 12
ABI_VERSION = 5

class LsnfRng(ctypes.Structure):
    """include/lsnf_flow.h `LsnfRng`: in-kernel Philox noise of lsnf_langevin_step and lsnf_sample."""
    _fields_ = [("seed", ctypes.c_uint64), ("offset", ctypes.c_uint64), ("offset_dev", c_void_p), ("row0", ctypes.c_int64)]


class LsnfDualAvg(ctypes.Structure):
    """include/lsnf_flow_mcmc.h `LsnfDualAvg`: the constants of the dual averaging of lsnf_hmc_step_rows' steps."""
    _fields_ = [("target_accept", c_float), ("gamma", c_float), ("t0", c_float), ("kappa", c_float), ("step_min", c_float),
                ("step_max", c_float)]


class LsnfMetricReg(ctypes.Structure):
    """include/lsnf_flow_mcmc.h `LsnfMetricReg`: the constants with which lsnf_hmc_step_metric closes a warm-up window."""
    _fields_ = [("n0", c_float), ("var0", c_float), ("scale_min", c_float), ("scale_max", c_float)]


class LsnfAdamOptions(ctypes.Structure):
    """include/lsnf_flow.h `LsnfAdamOptions`: the arguments of lsnf_adam_step_ex."""
    _fields_ = [("struct_bytes", ctypes.c_uint), ("flags", ctypes.c_uint), ("lr", c_double), ("lr_dev", c_void_p),
                ("beta1", c_double), ("beta2", c_double), ("eps", c_double), ("weight_decay", c_double), ("max_norm", c_double),
                ("ema_decay", c_double), ("grad_norm_out", c_void_p)]


# name -> (restype, argtypes); mirrors include/lsnf_flow.h one to one
_SIGNATURES = {
    "lsnf_abi_version": (c_int, []),
    "lsnf_last_error": (c_char_p, []),
    "lsnf_set_small_batch_max": (c_int, [c_int]),
    "lsnf_set_math_mode": (c_int, [c_int]),
    "lsnf_device_arch": (c_int, [c_int, c_char_p, c_size_t]),
    "lsnf_plan_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "lsnf_prepare_scratch_bytes": (c_size_t, [c_int, c_int, c_int]),
    "lsnf_prepare": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "lsnf_actnorm_init_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "lsnf_actnorm_init": (c_int, [ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "lsnf_forward": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_params_fast_path": (c_int, []),
    "lsnf_act_saved_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "lsnf_restash": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_reverse": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_backward_z": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float, c_void_p, c_void_p]),
    "lsnf_reverse_backward_z": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_langevin_step": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(LsnfRng), c_float,
                                   c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_sample": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(LsnfRng), c_float,
                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_reverse_keep_covers": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "lsnf_reverse_keep": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_sample_keep": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(LsnfRng), c_float,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_reverse_langevin_step": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(LsnfRng), c_float,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_backward_params_workspace_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "lsnf_backward_params": (c_int, [c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p),
                                     c_int, c_int, c_int, c_int, c_int,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float,
                                     c_void_p, c_void_p, c_void_p]),
    "lsnf_backward_params_det_workspace_floats": (c_size_t, [c_int, c_int, c_int, c_int]),
    "lsnf_backward_params_det": (c_int, [c_void_p, ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p),
                                         c_int, c_int, c_int, c_int, c_int,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_float,
                                         c_void_p, c_void_p, c_void_p]),
    "lsnf_adam_state_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),
    "lsnf_adam_step": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_void_p,
                               c_double, c_void_p, c_double, c_double, c_double, c_double, c_double, c_void_p, c_void_p]),
    "lsnf_adam_state_bytes_ex": (c_size_t, [c_int, c_int, c_int, c_int, ctypes.c_uint]),
    "lsnf_adam_step_ex": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), c_int, c_int, c_int, c_int, c_void_p,
                                  ctypes.POINTER(LsnfAdamOptions), c_void_p]),
}

# the extensions of include/lsnf_flow_mcmc.h: exported by the same library, outside the core ABI's symbol set
_EXT_SIGNATURES = {
    "lsnf_mala_step": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, ctypes.POINTER(LsnfRng), c_float, ctypes.c_uint,
                               c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_reverse_mala_step": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, ctypes.POINTER(LsnfRng), c_float, ctypes.c_uint,
                                       c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_hmc_step": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, ctypes.POINTER(LsnfRng), c_float, ctypes.c_uint,
                              c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_reverse_hmc_step": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, ctypes.POINTER(LsnfRng), c_float, ctypes.c_uint,
                                      c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_hmc_step_rows": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, ctypes.POINTER(LsnfRng),
                                   c_void_p, c_void_p, ctypes.POINTER(LsnfDualAvg), ctypes.c_uint,
                                   c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_reverse_hmc_step_rows": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_void_p, ctypes.POINTER(LsnfRng),
                                           c_void_p, c_void_p, ctypes.POINTER(LsnfDualAvg), ctypes.c_uint,
                                           c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_hmc_step_metric": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, ctypes.POINTER(LsnfRng),
                                     c_void_p, c_void_p, ctypes.POINTER(LsnfDualAvg),
                                     c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(LsnfMetricReg), ctypes.c_uint,
                                     c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_reverse_hmc_step_metric": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, ctypes.POINTER(LsnfRng),
                                             c_void_p, c_void_p, ctypes.POINTER(LsnfDualAvg),
                                             c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(LsnfMetricReg), ctypes.c_uint,
                                             c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_hmc_step_tempered": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, ctypes.POINTER(LsnfRng),
                                       c_void_p, c_void_p, ctypes.POINTER(LsnfDualAvg),
                                       c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(LsnfMetricReg),
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_uint,
                                       c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_reverse_hmc_step_tempered": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, ctypes.POINTER(LsnfRng),
                                               c_void_p, c_void_p, ctypes.POINTER(LsnfDualAvg),
                                               c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(LsnfMetricReg),
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_uint,
                                               c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_hmc_step_exchange": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, ctypes.POINTER(LsnfRng),
                                       c_void_p, c_void_p, ctypes.POINTER(LsnfDualAvg),
                                       c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(LsnfMetricReg),
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_uint,
                                       c_void_p, c_void_p, c_void_p,
                                       c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_reverse_hmc_step_exchange": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, ctypes.POINTER(LsnfRng),
                                               c_void_p, c_void_p, ctypes.POINTER(LsnfDualAvg),
                                               c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(LsnfMetricReg),
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_uint,
                                               c_void_p, c_void_p, c_void_p,
                                               c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_hmc_step_resample": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, ctypes.POINTER(LsnfRng),
                                       c_void_p, c_void_p, ctypes.POINTER(LsnfDualAvg),
                                       c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(LsnfMetricReg),
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_uint,
                                       c_void_p, c_void_p, c_void_p,
                                       c_int, ctypes.c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_reverse_hmc_step_resample": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, ctypes.POINTER(LsnfRng),
                                               c_void_p, c_void_p, ctypes.POINTER(LsnfDualAvg),
                                               c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(LsnfMetricReg),
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_uint,
                                               c_void_p, c_void_p, c_void_p,
                                               c_int, ctypes.c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "lsnf_hmc_step_schedule": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, ctypes.POINTER(LsnfRng),
                                       c_void_p, c_void_p, ctypes.POINTER(LsnfDualAvg),
                                       c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(LsnfMetricReg),
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_uint,
                                       c_void_p, c_void_p, c_void_p,
                                       c_int, ctypes.c_float, c_void_p, c_void_p, c_void_p, ctypes.c_float, ctypes.c_float, c_void_p]),
    "lsnf_reverse_hmc_step_schedule": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, ctypes.POINTER(LsnfRng),
                                               c_void_p, c_void_p, ctypes.POINTER(LsnfDualAvg),
                                               c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(LsnfMetricReg),
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_uint,
                                               c_void_p, c_void_p, c_void_p,
                                               c_int, ctypes.c_float, c_void_p, c_void_p, c_void_p, ctypes.c_float, ctypes.c_float, c_void_p]),
}

_lib = None


class LsnfError(RuntimeError):
    """A call into liblsnf_flow.so returned a negative status."""


def exported_symbols():
    return sorted(_SIGNATURES)


def extension_symbols():
    return sorted(_EXT_SIGNATURES)


def load():
    """dlopen the in-tree library and attach signatures.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LsnfError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C latent-space-normalizing-flow_amd/csrc`). There is no CPU/PyTorch fallback.")
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_LOCAL)
    for name, (res, args) in list(_SIGNATURES.items()) + list(_EXT_SIGNATURES.items()):
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    v = lib.lsnf_abi_version()
    if v != ABI_VERSION:
        raise LsnfError(f"liblsnf_flow.so ABI {v} != binding ABI {ABI_VERSION}: rebuild")
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != 0:
        msg = load().lsnf_last_error()
        raise LsnfError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")
