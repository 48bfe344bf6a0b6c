"""A counting stand-in for the object `lsnf_amd._lib.load()` returns: every call goes through to the real library and is counted
by name, so that a test can show that an argument check refused a call before any entry point that launches was entered."""
import collections

# entry points that only answer a question about sizes, modes or the build: they touch no device memory and launch nothing
QUERIES = frozenset((
    "lsnf_abi_version", "lsnf_last_error", "lsnf_set_small_batch_max", "lsnf_set_math_mode", "lsnf_device_arch", "lsnf_plan_floats",
    "lsnf_prepare_scratch_bytes", "lsnf_actnorm_init_workspace_bytes", "lsnf_params_fast_path", "lsnf_act_saved_floats",
    "lsnf_reverse_keep_covers", "lsnf_backward_params_workspace_floats", "lsnf_adam_state_bytes"))


class CountingLib:
    def __init__(self, real):
        self._real, self.entered = real, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def counted(*args):
            self.entered[name] += 1
            return fn(*args)
        return counted

    def launching(self):
        """Names of the entered entry points that may launch (everything but the queries)."""
        return sorted(n for n in self.entered if n not in QUERIES)


def install(monkeypatch, lsnf_amd):
    """Put a CountingLib in place of the loaded library for the rest of the test; returns it."""
    stand = CountingLib(lsnf_amd.load_library())
    monkeypatch.setattr(lsnf_amd._lib, "load", lambda: stand)
    return stand
