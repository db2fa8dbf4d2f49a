"""Gains, shapes and expected values of the mixdown per channel (mlgpu_bank_process_mixdown_channels and its listed and shard forms),
shared by tests/test_mixdown_channels_cpu.py and tests/test_gpu_mixdown_channels.py.

The one rule: channel c is the one-channel mixdown with the gains of channel c. So the expected values are the CPU checker's
chain_process per voice, then the checker's mixdown(y, gains[c]) per channel - nothing else."""
import numpy as np

from bank_groups_cases import T, Chain, special_gains

C = 2
# (V, chain): a wavefront and a quarter (spare lanes in the tree); nine workgroups through the XCD remap and a last one of 48 voices;
# 65 first-stage groups, so that each channel's region goes through two levels of the tree
SHAPES = ((80, "saw"), (80, "saw_odd"), (2352, "saw"), (2352, "saw_odd"), (4160, "saw"))
SPLITS = ((T,), (1, T - 1))
HARD_RIGHT, NEGATIVE_RIGHT = 2, 9   # voices: left gain 0.0 and right gain exactly 1.0; a negative right gain


def channel_gains(V):
    """[2][V] float32. gains[0] = special_gains(V) (a -0.0, a 0.0 and a denormal among them), gains[1] its constant-power partner
    sqrt(1 - g^2) in float32 - exactly 1.0 where the left gain is a zero or the denormal, which voice HARD_RIGHT (left gain +0.0) is
    - with the sign of voice NEGATIVE_RIGHT turned."""
    left = special_gains(V)
    right = np.sqrt(np.float32(1.0) - left * left).astype(np.float32)
    right[NEGATIVE_RIGHT] = -right[NEGATIVE_RIGHT]
    assert left[HARD_RIGHT].view(np.uint32) == 0 and right[HARD_RIGHT] == np.float32(1.0) and right[NEGATIVE_RIGHT] < 0
    assert np.isfinite(right).all()
    return np.ascontiguousarray(np.stack([left, right]))


def expected_channels(oracle, y, gains, flush=False):
    """y [V][S], the checker's voices -> [2][S]: the checker's mixdown tree once per channel."""
    with oracle.flush_denormals(flush):
        return np.stack([oracle.mixdown(y, np.ascontiguousarray(gains[c])) for c in range(gains.shape[0])])


_cases = {}


def case(oracle, name, V, flush=False):
    """(chain, gains [2][V], the voices [V][64 T], the channels [2][64 T], the state after) from clear(), once per case, read-only."""
    key = (name, V, flush)
    if key not in _cases:
        ch = Chain(name, oracle, V, 1)
        y, st = ch.oracle_voices(oracle, flush)
        gains = channel_gains(V)
        want = expected_channels(oracle, y, gains, flush)
        for a in (y, st, gains, want):
            a.setflags(write=False)
        _cases[key] = (ch, gains, y, want, st)
    return _cases[key]
