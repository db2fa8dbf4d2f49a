"""The group sums per channel without a GPU: the entry points as the header declares them, a guard on the GPU tests' own data, and the
lane plan, which the two-channel listed call shares with the one-channel one."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from groups_channels_cases import (C, CHAINS, GROUPS, LISTED_CASES, LISTED_V, VOICES, case, expected_channels, expected_group_sums,
                                   expected_listed_channels, expected_listed_groups, group_lists, listed_case)
from voice_list_groups_cases import PLAN_TABLE, model_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madronalib_amd", "csrc")
C_TO_CTYPES = {"mlgpu_bank*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "uint32_t*": ctypes.c_void_p,
               "size_t": ctypes.c_size_t, "int": ctypes.c_int}
DECLARED = {
    "mlgpu_bank_process_groups_channels": ["b", "n_vectors", "d_in", "in_layout", "in_group", "n_channels", "d_gains", "out_group", "d_out", "out_layout"],
    "mlgpu_bank_process_listed_groups_channels": ["b", "n_vectors", "d_in", "in_layout", "in_group", "n_channels", "d_gains", "d_out", "out_layout", "d_peak"],
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_entry_points_are_exported_and_declared_like_the_header():
    """The two symbols: exported by the library, declared in _lib.py with the header's parameter names and types, present in mlgpu.h.
    The change is additive, so the ABI version stays 2."""
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
    for method in ("process_groups_channels", "process_listed_groups_channels"):
        assert callable(getattr(ml.Bank, method))


def test_null_bank_is_refused_without_a_device():
    from madronalib_amd import _lib
    L = _lib.load()
    assert L.mlgpu_bank_process_groups_channels(None, 1, None, 0, 1, 2, None, 16, None, 0) == 1   # MLGPU_ERR_INVALID
    assert L.mlgpu_bank_process_listed_groups_channels(None, 1, None, 0, 1, 2, None, None, 0, None) == 1


@pytest.mark.parametrize("V", VOICES)
@pytest.mark.parametrize("name,in_group", CHAINS)
def test_the_channels_of_the_plain_cases_differ_from_each_other_and_from_the_plain_sums(oracle, name, in_group, V):
    """A vacuity guard: with these gains the CPU checker's two channels differ from each other and from the group sums without gains,
    at every group size - so a device call that returned one channel twice, or ignored the gains, could not pass the GPU tests."""
    ch, gains, y, _ = case(oracle, name, V, in_group)
    assert gains.shape == (C, V) and ch.in_group == in_group and (ch.in_rows is None) == (name != "streamed")
    for G in GROUPS:
        want = expected_channels(oracle, y, G, gains)
        plain = expected_group_sums(oracle, y, G)
        assert want.shape == (C, V // G, y.shape[1]) and np.isfinite(want).all() and np.abs(want).max() > 1e-6
        assert (bits(want[0]) != bits(want[1])).any(), "the two channels are the same"
        assert (bits(want[0]) != bits(plain)).any() and (bits(want[1]) != bits(plain)).any(), "a channel equals the sums without gains"
        # every instrument's two rows differ, not only some: the first voice of each group has two different gains
        assert (bits(want[0]) != bits(want[1])).any(axis=1).all(), "an instrument has the same row in both channels"


@pytest.mark.parametrize("lname,G,name,in_group,flush", LISTED_CASES)
def test_the_channels_of_the_listed_cases_differ_from_each_other_and_from_the_plain_sums(oracle, lname, G, name, in_group, flush):
    ch, gains, L, _, y, _ = listed_case(oracle, lname, name, in_group, flush)
    want, M = expected_listed_channels(oracle, y, L, G, gains, flush)
    plain, _ = expected_listed_groups(oracle, y, L, G, None, flush)
    assert want.shape == (C, M.size, y.shape[1])
    if L.size == 0:
        assert M.size == 0
        return
    assert np.isfinite(want).all() and np.abs(want).max() > 1e-6
    assert (bits(want[0]) != bits(want[1])).any(), "the two channels are the same"
    assert (bits(want[0]) != bits(plain)).any() and (bits(want[1]) != bits(plain)).any(), "a channel equals the sums without gains"


def test_the_lane_plan_is_the_one_channel_calls(tmp_path):
    """The two-channel listed call runs by the plan mlgpu_bank_set_voice_list makes for the one-channel call: nothing of it depends on
    the channel count. The planner (voice_list.cpp, built here with g++ alone) still gives the modelled table of lanes, pads and
    instruments on the lists of the GPU cases, and the model gives PLAN_TABLE."""
    lists = group_lists()
    for lname, G, *_ in LISTED_CASES:
        lanes, N, pads, J = model_plan(lists[lname], G)
        if (lname, G) in PLAN_TABLE:
            assert (N, pads, J) == PLAN_TABLE[(lname, G)], (lname, G)
        assert N - pads == lists[lname].size and N <= 64 * -(-lists[lname].size // (65 - G))
    assert {(n, g) for n, g, *_ in LISTED_CASES} >= {("straddle", 16), ("fit", 16), ("all", 16), ("k2100", 2), ("k2100", 4), ("k2100", 8)}
    exe =str(tmp_path / "listed_groups_plan_test")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(ROOT, "tests", "cpp", "listed_groups_plan_test.cpp"), os.path.join(CSRC, "voice_list.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    text = tmp_path / "lists.txt"
    text.write_text("".join(f"{name} {L.size} {' '.join(str(int(v)) for v in L)}\n" for name, L in lists.items()))
    r = subprocess.run([exe, str(text)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert LISTED_V == 2352
