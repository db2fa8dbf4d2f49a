"""Expected values and cases of the listed group sum (mlgpu_bank_reserve_voice_list_groups, mlgpu_bank_process_listed_groups), shared by
tests/test_voice_list_groups_cpu.py and tests/test_gpu_voice_list_groups.py.

The rule: the bank's voices are instruments of G adjacent voices; with the list L in force the call gives one row per LISTED
instrument - the distinct L[i] // G, ascending - which is ((0 + g y[a0]) + g y[a1]) + ... over that instrument's listed voices in voice
order, y the float mlgpu_bank_process_listed stores. So the expected rows are voice_list_cases.expected_listed's rows, each times its
voice's gain, accumulated per segment from +0.0 with the CPU checker's float32 add."""
import numpy as np

from bank_groups_cases import T, Chain, expected_group_sums, special_gains   # noqa: F401  (the tests take them from here)
from madronalib_amd.constants import Op
from voice_list_cases import V, expected_listed, expected_peaks, make_chain, voice_lists   # noqa: F401

GROUPS = (2, 4, 8, 16)
WAVE = 64
PAD = 0xFFFFFFFF
# N (lanes), pads and J of the lane plan, modelled on the CPU for V = 2352
PLAN_TABLE = {
    ("k2100", 2): (2120, 20, 1167),
    ("k2100", 4): (2140, 40, 587),
    ("k2100", 8): (2212, 112, 294),
    ("k2100", 16): (2348, 248, 147),
    ("straddle", 16): (76, 2, 71),
    ("fit", 16): (81, 0, 63),
    ("all", 16): (2352, 0, 147),
}


def group_lists(V=V):
    """voice_lists()'s last, k80, k2100, all and empty, and two lists made for the 64-lane boundary at G = 16:
    straddle (K = 74): the four voices of instrument 62 sit at list positions 62 .. 65 - the segment does not fit, two pads;
    fit (K = 81): a segment ends exactly at lane 63 and a full 16-voice segment follows with no pad."""
    base = voice_lists(V)
    lists = {k: base[k] for k in ("last", "k80", "k2100", "all", "empty")}
    lists["straddle"] = np.array([16 * c + 3 for c in range(62)] + [992 + k for k in (1, 5, 9, 14)] + [16 * c + 7 for c in range(63, 71)], np.uint32)
    lists["fit"] = np.array([16 * c + 3 for c in range(60)] + list(range(960, 964)) + list(range(976, 992)) + [1007], np.uint32)
    return lists


def listed_instruments(L, G):
    """M: the distinct L[i] // G, ascending (uint32), and for every list position the row of its instrument."""
    c = np.asarray(L, np.int64) // G
    M, row = np.unique(c, return_inverse=True)
    return M.astype(np.uint32), row.reshape(-1)


def model_plan(L, G):
    """The lane plan as the header states it, in plain Python: (voice-or-PAD per lane [N], N, pads, J)."""
    L = [int(v) for v in L]
    lanes = []
    i = J = 0
    while i < len(L):
        n = 1
        while i + n < len(L) and L[i + n] // G == L[i] // G:
            n += 1
        room = WAVE - len(lanes) % WAVE
        if n > room:
            lanes += [PAD] * room
        lanes += L[i:i + n]
        i += n
        J += 1
    return lanes, len(lanes), sum(1 for v in lanes if v == PAD), J


def expected_listed_groups(oracle, y, L, G, gains=None, flush=False):
    """y [K][S]: expected_listed's rows of the list L -> (rows [J][S] float32, M [J] uint32). Gains are indexed by VOICE (None: no
    multiply); every operation is the checker's float32 one under its flush-denormals mode when `flush`."""
    y = np.ascontiguousarray(y, np.float32)
    K, S = y.shape
    L = np.asarray(L, np.int64)
    assert L.size == K
    M, row = listed_instruments(L, G)
    J = M.size
    acc = np.zeros((J, S), np.float32)   # +0.0
    if K == 0:
        return acc, M
    rank = np.arange(K) - np.searchsorted(row, row, side="left")   # the voice's place among its instrument's listed voices
    g = None if gains is None else np.ascontiguousarray(np.repeat(np.asarray(gains, np.float32)[L][:, None], S, axis=1))
    with oracle.flush_denormals(flush):   # (checker calls and copies only: numpy arithmetic on this thread would see the mode too)
        if g is not None:
            y = oracle.op_f32(Op.MULTIPLY, y, g)
        for r in range(int(rank.max()) + 1):
            at = np.nonzero(rank == r)[0]
            rows = row[at]
            acc[rows] = oracle.op_f32(Op.ADD, np.ascontiguousarray(acc[rows]), np.ascontiguousarray(y[at]))
    return acc, M
