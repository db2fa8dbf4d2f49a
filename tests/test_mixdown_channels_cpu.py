"""The mixdown per channel without a GPU: the entry points as the header declares them, and a guard on the GPU tests' own data."""
import ctypes
import os
import re

import numpy as np

from mixdown_channels_cases import HARD_RIGHT, NEGATIVE_RIGHT, case, channel_gains

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TO_CTYPES = {"mlgpu_bank*": ctypes.c_void_p, "mlgpu_engine*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p,
               "uint32_t*": ctypes.c_void_p, "size_t": ctypes.c_size_t, "int": ctypes.c_int}
DECLARED = {
    "mlgpu_mixdown_reserve_channels": ["e", "max_voices", "max_vectors", "max_channels"],
    "mlgpu_mixdown_channels": ["e", "d_signal", "layout", "n_voices", "n_vectors", "n_channels", "d_gains", "d_out"],
    "mlgpu_bank_process_mixdown_channels": ["bank", "n_vectors", "d_in", "in_layout", "n_channels", "d_gains", "d_out"],
    "mlgpu_bank_process_mixdown_channels_shard": ["bank", "n_vectors", "d_in", "in_layout", "n_channels", "d_gains", "d_rows"],
    "mlgpu_bank_process_listed_mixdown_channels": ["bank", "n_vectors", "d_in", "in_layout", "n_channels", "d_gains", "d_out", "d_peak"],
}


def test_entry_points_are_exported_and_declared_like_the_header():
    """The five symbols: exported by the library, declared in _lib.py with the header's parameter types, present in mlgpu.h. The change
    is additive, so the ABI version stays 2."""
    from madronalib_amd import _lib
    L = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mlgpu.h")).read(), flags=re.S)
    declared = open(os.path.join(ROOT, "madronalib_amd", "_lib.py")).read()
    for name, want_names in DECLARED.items():
        fn = getattr(L, name)   # AttributeError: not exported
        assert f'sig("{name}"' in declared, f"madronalib_amd/_lib.py does not declare {name}"
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"include/mlgpu.h does not declare {name}"
        params = [" ".join(p.split()) for p in m.group(2).split(",")]
        assert [p.split()[-1] for p in params] == want_names, name
        assert m.group(1) == "int" and fn.restype is ctypes.c_int, name
        assert [C_TO_CTYPES[p.rsplit(" ", 1)[0]] for p in params] == list(fn.argtypes), name
    assert L.mlgpu_abi_version() == 2
    import madronalib_amd as ml
    for method in ("mixdown_reserve_channels", "mixdown_channels"):
        assert callable(getattr(ml.Engine, method))
    for method in ("process_mixdown_channels", "process_mixdown_channels_shard", "process_listed_mixdown_channels"):
        assert callable(getattr(ml.Bank, method))


def test_the_gains_have_what_the_gpu_tests_say_they_have():
    for V in (80, 2352, 4160):
        g = channel_gains(V)
        assert g.shape == (2, V) and g.dtype == np.float32
        bits = g[0].view(np.uint32)
        assert (bits == 0x80000000).any() and (bits == 0).any() and ((bits & 0x7F800000 == 0) & (bits & 0x007FFFFF != 0)).any()
        assert bits[HARD_RIGHT] == 0 and g[1, HARD_RIGHT] == np.float32(1.0) and g[1, NEGATIVE_RIGHT] < 0


def test_the_channels_of_the_test_data_differ_from_each_other_and_from_the_plain_mix(oracle):
    """A vacuity guard: with these gains the CPU checker's two channels differ from each other and from the unscaled mix - so a device
    call that returned one channel twice, or ignored the gains, could not pass the GPU tests."""
    for V, name in ((80, "saw"), (80, "saw_odd"), (2352, "saw")):
        ch, gains, y, want, _ = case(oracle, name, V)
        plain = oracle.mixdown(y, None)
        u = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
        assert np.isfinite(want).all() and np.abs(want).max() > 1e-6
        assert (u(want[0]) != u(want[1])).any(), "the two channels are the same"
        assert (u(want[0]) != u(plain)).any() and (u(want[1]) != u(plain)).any(), "a channel equals the unscaled mix"
