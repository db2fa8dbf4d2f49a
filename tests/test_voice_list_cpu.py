"""Voice lists without a GPU: the host check of a list (madronalib_amd/csrc/voice_list.cpp, plain C++ driven by
tests/cpp/voice_list_test.cpp), the entry points as the header declares them, and the expected-value helpers of the GPU tests
against themselves."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from bank_groups_cases import T
from voice_list_cases import CHAINS, V, expected_listed, expected_listed_mixdown, expected_peaks, make_chain, voice_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madronalib_amd", "csrc")
C_TO_CTYPES = {"mlgpu_bank*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "const uint32_t*": ctypes.c_void_p,
               "uint32_t*": ctypes.c_void_p, "size_t": ctypes.c_size_t, "int": ctypes.c_int}
DECLARED = {
    "mlgpu_bank_reserve_voice_list": ("int", ["b", "max_listed"]),
    "mlgpu_bank_set_voice_list": ("int", ["b", "h_voices", "n"]),
    "mlgpu_bank_voice_list_size": ("size_t", ["b"]),
    "mlgpu_bank_process_listed": ("int", ["b", "n_vectors", "d_in", "in_layout", "d_out", "out_layout", "d_peak"]),
    "mlgpu_bank_process_listed_mixdown": ("int", ["b", "n_vectors", "d_in", "in_layout", "d_gains", "d_out", "d_peak"]),
}


def test_list_validation_on_the_cpu(tmp_path):
    """voice_list.cpp is plain C++: built by g++ from that one file with no HIP include path. Ascending and empty lists accepted; an
    equal neighbour, a descending pair and an out-of-range index refused with the position in the message; a list longer than the
    reserve refused (tests/cpp/voice_list_test.cpp)."""
    if not os.path.exists("/usr/bin/g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "voice_list_test")
    src = os.path.join(CSRC, "voice_list.cpp")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", os.path.join(ROOT, "tests", "cpp", "voice_list_test.cpp"), src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    used = subprocess.run(["g++", "-std=c++17", "-M", src], capture_output=True, text=True, timeout=300).stdout
    assert "hip/" not in used and "hip_runtime" not in used and "voice_list.hpp" in used
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_entry_points_are_exported_and_declared_like_the_header():
    from madronalib_amd import _lib
    L = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mlgpu.h")).read(), flags=re.S)
    for name, (res, want_names) in DECLARED.items():
        fn = getattr(L, name)   # AttributeError: not exported
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"include/mlgpu.h does not declare {name}"
        params = [" ".join(p.split()) for p in m.group(2).split(",")]
        assert [p.split()[-1] for p in params] == want_names, name
        assert m.group(1) == res
        assert [C_TO_CTYPES[p.rsplit(" ", 1)[0]] for p in params] == list(fn.argtypes), name
        assert fn.restype is C_TO_CTYPES[res], name
    assert L.mlgpu_abi_version() == 2   # additive: the version stays
    import madronalib_amd as ml
    for method in ("reserve_voice_list", "set_voice_list", "process_listed", "process_listed_mixdown"):
        assert callable(getattr(ml.Bank, method))


def test_null_bank_is_refused_without_a_device():
    from madronalib_amd import _lib
    L = _lib.load()
    assert L.mlgpu_bank_reserve_voice_list(None, 4) == 1   # MLGPU_ERR_INVALID
    assert L.mlgpu_bank_set_voice_list(None, None, 0) == 1
    assert L.mlgpu_bank_voice_list_size(None) == 0
    assert L.mlgpu_bank_process_listed(None, 1, None, 0, None, 0, None) == 1
    assert L.mlgpu_bank_process_listed_mixdown(None, 1, None, 0, None, None, None) == 1


def test_the_cases_are_what_the_kernel_needs():
    lists = voice_lists()
    assert [lists[k].size for k in ("last", "wave", "k80", "k2100", "all", "empty")] == [1, 64, 80, 2100, V, 0]
    assert lists["last"][0] == V - 1 and lists["wave"][-1] == 2331 and (np.diff(lists["wave"]) == 37).all()
    for name, L in lists.items():
        assert L.dtype == np.uint32 and (np.diff(L.astype(np.int64)) > 0).all() and (L < V).all(), name
    for name in ("k80", "k2100", "all"):
        assert 5 in lists[name] and V - 3 in lists[name], name     # saw_odd's slow-head lanes stay listed
    assert (2100 + 255) // 256 == 9 and 2100 - 8 * 256 == 52      # eight remapped workgroups and a last one of 52 lanes


@pytest.mark.parametrize("name", CHAINS)
def test_a_list_of_every_voice_is_the_plain_oracle_run(oracle, name):
    """expected_listed with L = range(V) - in one run, and in runs of 1 + 2 DSPVectors - gives the output and the state of the plain
    oracle run the bank tests use (Chain.oracle_voices); a partial list gives those voices' rows of it and leaves every other state
    column alone; the peaks and the mixdown of the helpers follow from the rows."""
    ch = make_chain(oracle, name)
    want, want_state = ch.oracle_voices(oracle)
    everyone = np.arange(V)
    st = oracle.chain_clear(ch.procs, V)
    got = expected_listed(oracle, ch, everyone, st)
    assert (got.view(np.uint32) == want.view(np.uint32)).all() and (st == want_state).all()
    st = oracle.chain_clear(ch.procs, V)
    split = np.concatenate([expected_listed(oracle, ch, everyone, st, 0, 1), expected_listed(oracle, ch, everyone, st, 1, T - 1)], 1)
    assert (split.view(np.uint32) == want.view(np.uint32)).all() and (st == want_state).all()
    # the voices of a chain are independent: a partial list gives those rows, and time passes for nobody else
    L = voice_lists()["k80"].astype(np.int64)
    clear = oracle.chain_clear(ch.procs, V)
    st = clear.copy()
    part = expected_listed(oracle, ch, L, st)
    assert (part.view(np.uint32) == want[L].view(np.uint32)).all()
    rest = np.setdiff1d(everyone, L)
    assert (st[:, L] == want_state[:, L]).all() and (st[:, rest] == clear[:, rest]).all()
    peaks = expected_peaks(part)
    assert peaks.dtype == np.uint32 and (peaks == np.abs(part).max(axis=1).view(np.uint32)).all()
    assert (expected_listed_mixdown(oracle, part, L).view(np.uint32) == oracle.mixdown(np.ascontiguousarray(want[L])).view(np.uint32)).all()


def test_helpers_on_the_empty_list_and_on_special_values(oracle):
    ch = make_chain(oracle, "saw")
    st = oracle.chain_clear(ch.procs, V)
    before = st.copy()
    y = expected_listed(oracle, ch, [], st)
    assert y.shape == (0, 64 * T) and (st == before).all()
    assert expected_peaks(y).shape == (0,)
    assert (expected_listed_mixdown(oracle, y, []).view(np.uint32) == 0).all()          # +0.0, not -0.0
    rows = np.array([[0.0, -0.0, 1e-40, -2.0], [np.nan, 1.0, -np.inf, 0.0], [-0.0, 0.0, 0.0, -0.0]], np.float32)
    peaks = expected_peaks(rows)
    assert peaks[0] == np.float32(2.0).view(np.uint32) and peaks[1] > 0x7F800000 and peaks[2] == 0
