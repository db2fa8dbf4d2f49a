"""Gains, chains and expected values of the group sums per channel (mlgpu_bank_process_groups_channels and
mlgpu_bank_process_listed_groups_channels), shared by tests/test_groups_channels_cpu.py and tests/test_gpu_groups_channels.py.

The one rule: channel c is the one-channel call with the gains of channel c. So the expected channels are
bank_groups_cases.expected_group_sums / voice_list_groups_cases.expected_listed_groups, called once per channel with gains[c] and
nothing else; the gains are mixdown_channels_cases.channel_gains (a -0.0, a 0.0, a denormal, a hard-right voice and a negative
right gain among them)."""
import numpy as np

from bank_groups_cases import T, VOICES, Chain, expected_group_sums
from mixdown_channels_cases import channel_gains
from voice_list_cases import V as LISTED_V, chain_inputs, expected_listed, expected_peaks
from voice_list_groups_cases import expected_listed_groups, group_lists

C = 2
GROUPS = (2, 4, 8, 16)
# (chain, in_group): SawGen -> Bandpass -> Gain on per-voice constant frequencies with the fast head (saw) and with two lanes that
# send their wavefronts to the slow head (saw_odd), and on a STREAMED frequency of V / in_group rows (HAS_SIGNAL, the input group)
CHAINS = (("saw", 1), ("saw_odd", 1), ("streamed", 1), ("streamed", 4))
SPLITS = ((T,), (1, T - 1))
# (list, G, chain, in_group, flush) of the listed call over V = 2352: the lists made for the 64-lane boundary, a wavefront and a
# quarter, the last voice alone, every voice and none at G = 16; 248, 40 and 112 pad lanes over ten workgroups at G = 2, 4, 8
LISTED_CASES = (("straddle", 16, "saw", 1, False), ("fit", 16, "saw_odd", 1, False), ("k80", 16, "streamed", 4, False), ("last", 16, "saw", 1, False),
                ("all", 16, "saw_odd", 1, True), ("empty", 16, "saw", 1, False),
                ("k2100", 2, "saw", 1, False), ("k2100", 4, "streamed", 1, True), ("k2100", 8, "saw_odd", 1, False))


class StreamedSaw(Chain):
    """SawGen -> Bandpass -> Gain with saw's coefficients, the frequency STREAMED: V / in_group rows, row r holding
    55 * 2^(5 r / R) / 48000 in every sample of the launch - so that the checker's chain_process needs nothing new."""

    def __init__(self, oracle, V, in_group):
        Chain.__init__(self, "saw", oracle, V, in_group)
        self.name = "streamed"
        R = V // in_group
        f = (55.0 * 2.0 ** (5.0 * np.arange(R) / R) / 48000.0).astype(np.float32)
        self.in_const = None
        self.in_rows = np.ascontiguousarray(np.repeat(f[:, None], 64 * T, axis=1))


def make_chain(oracle, name, V, in_group=1):
    return StreamedSaw(oracle, V, in_group) if name == "streamed" else Chain(name, oracle, V, in_group)


def expected_channels(oracle, y, G, gains, flush=False):
    """y [V][S], the checker's voices -> [2][V / G][S]: expected_group_sums once per channel."""
    return np.stack([expected_group_sums(oracle, y, G, np.ascontiguousarray(gains[c]), flush) for c in range(gains.shape[0])])


def expected_listed_channels(oracle, y, L, G, gains, flush=False):
    """y [K][S], the checker's listed voices -> ([2][J][S], M [J]): expected_listed_groups once per channel."""
    rows = [expected_listed_groups(oracle, y, L, G, np.ascontiguousarray(gains[c]), flush) for c in range(gains.shape[0])]
    return np.stack([r[0] for r in rows]), rows[0][1]


_cases = {}


def case(oracle, name, V, in_group=1, flush=False):
    """(chain, gains [2][V], the voices [V][64 T], the state after one pass) from clear(), once per case, read-only."""
    key = (name, V, in_group, flush)
    if key not in _cases:
        ch = make_chain(oracle, name, V, in_group)
        y, st = ch.oracle_voices(oracle, flush)
        gains = channel_gains(V)
        for a in (y, st, gains):
            a.setflags(write=False)
        _cases[key] = (ch, gains, y, st)
    return _cases[key]


_prepared, _listed = {}, {}


def prepared(oracle, name, in_group=1, flush=False):
    """(chain over voice_list_cases.V voices, the checker's state after one DSPVector of ALL voices from clear()): the state an
    unlisted voice must keep is then not the cleared one. Once per chain, input group and mode."""
    key = (name, in_group, flush)
    if key not in _prepared:
        ch = make_chain(oracle, name, LISTED_V, in_group)
        st0 = oracle.chain_clear(ch.procs, LISTED_V)
        x = chain_inputs(ch)
        with oracle.flush_denormals(flush):
            oracle.chain_process(ch.procs, 1, ch.coeffs, st0, None if x is None else np.ascontiguousarray(x[:, :64]), ch.in_const, n_threads=4, want_out=False)
        st0.setflags(write=False)
        _prepared[key] = (ch, st0)
    return _prepared[key]


def listed_case(oracle, lname, name, in_group=1, flush=False):
    """(chain, gains [2][V], the list, the state before, the listed voices' signals [K][64 T], the full state after) for one launch
    of T DSPVectors on the prepared bank, once per case, read-only."""
    key = (lname, name, in_group, flush)
    if key not in _listed:
        ch, st0 = prepared(oracle, name, in_group, flush)
        L = group_lists()[lname]
        st = st0.copy()
        y = expected_listed(oracle, ch, L, st, 0, T, flush)
        gains = channel_gains(LISTED_V)
        for a in (y, st, gains):
            a.setflags(write=False)
        _listed[key] = (ch, gains, L, st0, y, st)
    return _listed[key]


__all__ = ["C", "CHAINS", "GROUPS", "LISTED_CASES", "LISTED_V", "SPLITS", "T", "VOICES", "case", "chain_inputs", "channel_gains", "expected_channels",
           "expected_group_sums", "expected_listed_channels", "expected_listed_groups", "expected_peaks", "group_lists", "listed_case", "make_chain",
           "prepared"]
