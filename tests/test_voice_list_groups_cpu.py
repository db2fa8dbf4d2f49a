"""The listed group sum without a GPU: the host's lane plan (madronalib_amd/csrc/voice_list.cpp: mlvl::planGroups, plain C++ driven by
tests/cpp/listed_groups_plan_test.cpp under the sanitizers), the entry points as the header declares them, and the expected-value
helpers of the GPU tests against themselves."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from voice_list_groups_cases import (GROUPS, PAD, PLAN_TABLE, T, V, expected_group_sums, expected_listed, expected_listed_groups, group_lists,
                                     listed_instruments, make_chain, model_plan, special_gains)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madronalib_amd", "csrc")
C_TO_CTYPES = {"mlgpu_bank*": ctypes.c_void_p, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p, "const uint32_t*": ctypes.c_void_p,
               "uint32_t*": ctypes.c_void_p, "size_t": ctypes.c_size_t, "int": ctypes.c_int}
DECLARED = {
    "mlgpu_bank_reserve_voice_list_groups": ("int", ["b", "max_listed", "out_group"]),
    "mlgpu_bank_listed_group_count": ("size_t", ["b"]),
    "mlgpu_bank_listed_groups": ("int", ["b", "h_groups", "capacity"]),
    "mlgpu_bank_process_listed_groups": ("int", ["b", "n_vectors", "d_in", "in_layout", "in_group", "d_gains", "d_out", "out_layout", "d_peak"]),
}


def test_lane_plan_under_sanitizers(tmp_path):
    """tests/cpp/listed_groups_plan_test.cpp: the plan's facts on the named lists at G = 2, 4, 8, 16 with the modelled table of
    N / pads / J, on every voice of banks of whole groups and on 2 000 seeded random lists; built with g++
    -fsanitize=address,undefined from voice_list.cpp alone - no HIP include path - and run directly."""
    if not os.path.exists("/usr/bin/g++"):
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    pb = subprocess.run(["g++", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=300)
    if pb.returncode != 0:
        pytest.skip("sanitizer runtime not installed: " + pb.stderr[-200:])
    exe = str(tmp_path / "listed_groups_plan_test")
    src = os.path.join(CSRC, "voice_list.cpp")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cpp", "listed_groups_plan_test.cpp"), src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    used = subprocess.run(["g++", "-std=c++17", "-M", src], capture_output=True, text=True, timeout=300).stdout
    assert "hip/" not in used and "hip_runtime" not in used and "voice_list.hpp" in used
    lists = tmp_path / "lists.txt"
    lists.write_text("".join(f"{name} {L.size} {' '.join(str(int(v)) for v in L)}\n" for name, L in group_lists().items()))
    r = subprocess.run([exe, str(lists)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
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
    for method in ("reserve_voice_list_groups", "process_listed_groups"):
        assert callable(getattr(ml.Bank, method))
    assert isinstance(ml.Bank.listed_groups, property)


def test_null_bank_is_refused_without_a_device():
    from madronalib_amd import _lib
    L = _lib.load()
    assert L.mlgpu_bank_reserve_voice_list_groups(None, 4, 16) == 1   # MLGPU_ERR_INVALID
    assert L.mlgpu_bank_listed_group_count(None) == 0
    m = np.zeros(4, np.uint32)
    assert L.mlgpu_bank_listed_groups(None, m.ctypes.data_as(ctypes.c_void_p), 4) == 1
    assert L.mlgpu_bank_process_listed_groups(None, 1, None, 0, 1, None, None, 0, None) == 1


def test_the_cases_are_what_the_kernel_needs():
    lists = group_lists()
    assert [lists[k].size for k in ("last", "k80", "k2100", "all", "empty", "straddle", "fit")] == [1, 80, 2100, V, 0, 74, 81]
    for name, L in lists.items():
        assert L.dtype == np.uint32 and (np.diff(L.astype(np.int64)) > 0).all() and (L < V).all(), name
    for name in ("k2100", "all"):
        assert 5 in lists[name] and V - 3 in lists[name], name     # saw_odd's slow-head lanes stay listed
    # straddle: instrument 62's four voices at list positions 62 .. 65; fit: a segment ends at lane 63, a full one follows
    s, f = lists["straddle"], lists["fit"]
    assert (s[62:66] // 16 == 62).all() and s[61] // 16 == 61 and s[66] // 16 == 63
    lanes, N, pads, J = model_plan(s, 16)
    assert lanes[62:64] == [PAD, PAD] and lanes[64:68] == [993, 997, 1001, 1006] and (N, pads, J) == (76, 2, 71)
    lanes, N, pads, J = model_plan(f, 16)
    assert lanes[60:64] == [960, 961, 962, 963] and lanes[64:80] == list(range(976, 992)) and (N, pads, J) == (81, 0, 63)
    # the modelled table, the reserve's bound, and the workgroups of the two big launches: ten, eight of them through the XCD remap
    for (name, G), want in PLAN_TABLE.items():
        lanes, N, pads, J = model_plan(lists[name], G)
        assert (N, pads, J) == want, (name, G)
        assert J == listed_instruments(lists[name], G)[0].size
    for name, L in lists.items():
        for G in GROUPS:
            N = model_plan(L, G)[1]
            assert N <= 64 * -(-L.size // (65 - G)), (name, G)
    for name in ("k2100", "all"):
        assert (model_plan(lists[name], 16)[1] + 255) // 256 == 10
    assert V % 16 == 0


@pytest.mark.parametrize("name", ("saw", "bandpass"))
def test_a_list_of_every_voice_gives_the_group_sums_of_the_plain_run(oracle, name):
    """expected_listed_groups on `all` equals expected_group_sums of the full oracle run bit for bit, with and without special_gains,
    at every group size and in both floating-point modes; a partial list gives the sums of the listed voices alone."""
    ch = make_chain(oracle, name)
    everyone = np.arange(V)
    for flush in (False, True):
        want, _ = ch.oracle_voices(oracle, flush)
        y = expected_listed(oracle, ch, everyone, oracle.chain_clear(ch.procs, V), flush=flush)
        assert (y.view(np.uint32) == want.view(np.uint32)).all()
        for G in GROUPS:
            for gains in (None, special_gains(V)):
                rows, M = expected_listed_groups(oracle, y, everyone, G, gains, flush)
                sums = expected_group_sums(oracle, want, G, gains, flush)
                assert rows.shape == sums.shape and (rows.view(np.uint32) == sums.view(np.uint32)).all(), (G, gains is None, flush)
                assert M.dtype == np.uint32 and (M == np.arange(V // G)).all()
    # a partial list: each row is the in-order sum of its instrument's listed voices, by hand in numpy (default mode, no denormals
    # in these signals' sums would change that: compare with the checker's add one segment at a time)
    from madronalib_amd.constants import Op
    L = group_lists()["straddle"].astype(np.int64)
    want, _ = ch.oracle_voices(oracle)
    rows, M = expected_listed_groups(oracle, want[L], L, 16)
    assert (M == np.unique(L // 16)).all() and rows.shape == (71, 64 * T)
    j = int(np.nonzero(M == 62)[0][0])
    acc = np.zeros(64 * T, np.float32)
    for v in (993, 997, 1001, 1006):
        acc = oracle.op_f32(Op.ADD, acc, np.ascontiguousarray(want[v]))
    assert (rows[j].view(np.uint32) == acc.view(np.uint32)).all()
    assert (rows[0].view(np.uint32) == oracle.op_f32(Op.ADD, np.zeros(64 * T, np.float32), np.ascontiguousarray(want[3])).view(np.uint32)).all()


def test_helpers_on_the_empty_list_and_on_special_values(oracle):
    rows, M = expected_listed_groups(oracle, np.zeros((0, 64 * T), np.float32), [], 16)
    assert rows.shape == (0, 64 * T) and M.shape == (0,)
    # a single -0.0 voice: 0 + -0.0 = +0.0
    y = np.full((1, 64 * T), -0.0, np.float32)
    assert (y.view(np.uint32) == 0x80000000).all()
    rows, M = expected_listed_groups(oracle, y, [37], 16)
    assert rows.shape == (1, 64 * T) and (rows.view(np.uint32) == 0).all() and list(M) == [2]
    # ... and a gain of -0.0 on a positive voice gives -0.0 before the add, +0.0 after
    gains = np.ones(V, np.float32)
    gains[37] = np.float32(-0.0)
    rows, _ = expected_listed_groups(oracle, np.ones((1, 64 * T), np.float32), [37], 16, gains)
    assert (rows.view(np.uint32) == 0).all()
    # a denormal gain under flush: the product's source reads as zero
    gains[37] = np.float32(1e-40)
    rows, _ = expected_listed_groups(oracle, np.ones((1, 64 * T), np.float32), [37], 2, gains, flush=True)
    assert (rows.view(np.uint32) == 0).all()
    rows, _ = expected_listed_groups(oracle, np.ones((1, 64 * T), np.float32), [37], 2, gains, flush=False)
    assert (rows == np.float32(1e-40)).all()
