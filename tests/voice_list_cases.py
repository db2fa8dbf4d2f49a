"""Expected values and cases of the voice-list calls (mlgpu_bank_set_voice_list, mlgpu_bank_process_listed, _listed_mixdown), shared by
tests/test_voice_list_cpu.py and tests/test_gpu_voice_list.py.

The one rule: a listed call behaves as a bank of K voices made of voices L[0] ... L[K-1]. So the expected values are the CPU checker's
chain_process run on K voices whose coefficients, input constant and input rows are gathered by L, with the state rows taken from and
scattered back into the full bank's state; the mixdown is the checker's mixdown of those K rows (gains gathered by L); the peaks are
numpy on the expected output's bits."""
import numpy as np

from bank_groups_cases import T, Chain

V = 2352       # nine full 256-voice workgroups and a last one of 48 voices
CHAINS = ("saw", "saw_odd", "bandpass", "impulse")
MIX_CHAINS = ("saw", "saw_odd")   # the chains of the cases with an ahead-of-time summing form (SawGen -> Bandpass -> Gain)


def voice_lists(V=V):
    """name -> ascending uint32 indices. The seeded random lists keep voices 5 and V - 3 (saw_odd's slow-head lanes)."""
    def random_list(K, seed):
        rest = np.setdiff1d(np.arange(V), [5, V - 3])
        pick = np.random.default_rng(seed).choice(rest, K - 2, replace=False)
        return np.sort(np.concatenate([pick, [5, V - 3]])).astype(np.uint32)
    return {
        "last": np.array([V - 1], np.uint32),                      # K = 1
        "wave": np.arange(0, 64 * 37, 37, dtype=np.uint32),        # K = 64: exactly one wavefront, voices 0, 37 ... 2331
        "k80": random_list(80, 80),                                # a wavefront and a quarter: spare lanes in the mix form
        "k2100": random_list(2100, 2100),                          # nine workgroups: eight through the XCD remap, a last one of 52 lanes
        "all": np.arange(V, dtype=np.uint32),                      # K = V: the plain bank
        "empty": np.zeros(0, np.uint32),                           # K = 0
    }


def chain_inputs(ch):
    """The streamed input as one row per voice of the bank ([V][64 T]), or None."""
    return None if ch.in_rows is None else np.ascontiguousarray(np.repeat(ch.in_rows, ch.in_group, axis=0))


def expected_listed(oracle, ch, L, state, t0=0, n=T, flush=False, coeffs=None, in_const=None):
    """The oracle on the K listed voices for DSPVectors [t0, t0 + n): `state` [NS][V] (the full bank's) is read at L and updated at L in
    place, every other column is left alone. Returns [K][64 n] float32. coeffs / in_const override the chain's (still [..][V])."""
    L = np.asarray(L, np.int64)
    K = L.size
    if K == 0:
        return np.zeros((0, 64 * n), np.float32)
    co = ch.coeffs if coeffs is None else coeffs
    ic = ch.in_const if in_const is None else in_const
    x = chain_inputs(ch)
    co_k = np.ascontiguousarray(co[:, L])
    ic_k = None if ic is None else np.ascontiguousarray(ic[L])
    x_k = None if x is None else np.ascontiguousarray(x[L, 64 * t0:64 * (t0 + n)])
    st_k = np.ascontiguousarray(state[:, L])
    with oracle.flush_denormals(flush):
        y = oracle.chain_process(ch.procs, n, co_k, st_k, x_k, ic_k, n_threads=4)
    state[:, L] = st_k
    return y


def expected_peaks(y):
    """[K][S] float32 -> [K] uint32: the largest bits(y) & 0x7fffffff of each row (0 for a row without samples)."""
    bits = np.ascontiguousarray(y, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return bits.max(axis=1).astype(np.uint32) if bits.shape[1] else np.zeros(bits.shape[0], np.uint32)


def expected_listed_mixdown(oracle, y, L, gains=None, flush=False):
    """The K-voice mixdown tree over the listed voices' signals y [K][S], the gains (indexed by VOICE) gathered by L. No voices: +0."""
    if y.shape[0] == 0:
        return np.zeros(y.shape[1], np.float32)
    g = None if gains is None else np.ascontiguousarray(np.asarray(gains, np.float32)[np.asarray(L, np.int64)])
    with oracle.flush_denormals(flush):
        return oracle.mixdown(y, g)


def make_chain(oracle, name, V=V):
    return Chain(name, oracle, V, 1)
