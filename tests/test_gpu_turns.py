"""The turns of a SIMD's wavefronts at the priority levels (mldsp_math.hpp: take_turns_by_clock) change when instructions issue and
never what they compute, and so does leaving them out: the kernels of a launch that goes out in parts carry
MLGPU_KFLAG_LONE_WAVEFRONTS where they are at most a workgroup per CU, read no clock and set no level (mldsp_kernels.hpp:
stream_voice). With and without, the bits are the CPU checker's and those of one plain launch.

Bank: SawGen -> Bandpass -> Gain, 8 192 voices - the smallest bank that launch-parts mode 3 cuts into four whole units of 2 048 voices
(8 workgroups each, fewer than the chip has CUs: every part carries the flag; mode 1 is one kernel that takes turns). Frequencies as
in smoke(), 55 Hz .. 1.76 kHz at 48 kHz, all inside (0, 1/16]: every wavefront takes the trip head. One lane of every wavefront just
above 1/16: the fast head; one lane of every wavefront at 1e-30, an odd input: the general head (which head each wavefront takes is
asserted from choose_head's own conditions before the device is touched). T = 1 (four turn points) and T = 3, two consecutive
launches each, outputs and final state. The mix form, an SVF cascade and a generated graph kernel, which all take turns, once each."""
import functools

import numpy as np
import pytest

from graph_oracle import evaluate
from inputs import assert_bits_equal, chain_coeffs, chain_input, gate_signal
from madronalib_amd.constants import Layout, Proc
from test_gpu_graph import build_synth16, synth16_setup

pytestmark = pytest.mark.gpu

V = 8192
SAW_BP_GAIN = [Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN]
HEADS = ["trip", "fast", "general"]
MODES = [1, 2, 3]                # mlgpu_engine_set_launch_parts: one kernel, two, four
CALLS = 2


@functools.lru_cache(maxsize=None)
def bank_coeffs():
    import madronalib_amd as ml
    freq = frequencies("trip")
    co = np.stack([ml.Bandpass.makeCoeffs(min(0.45, 4.0 * float(f)), 0.5) for f in freq], 1)  # [3][V]
    co = np.ascontiguousarray(np.concatenate([co, np.full((1, V), 0.25, np.float32)], 0))
    co.setflags(write=False)
    return co


@functools.lru_cache(maxsize=None)
def frequencies(head):
    freq = (55.0 * 2.0 ** (5.0 * np.arange(V) / V) / 48000.0).astype(np.float32)
    sixteenth = np.float32(1.0 / 16.0)
    assert ((freq > 0) & (freq <= sixteenth)).all()
    if head == "fast":
        freq[11::64] = np.nextafter(sixteenth, np.float32(1.0))
    if head == "general":
        freq[11::64] = np.float32(1e-30)      # positive and below 2^-64: an odd input (a frequency of 0 is not one)
    assert (heads_taken(freq) == head).all(), (head, np.unique(heads_taken(freq)))
    freq.setflags(write=False)
    return freq


def heads_taken(freq):
    """The head loop each wavefront of 64 voices takes, as choose_head decides it (mldsp_kernels.hpp) from blep_freq_is_odd and
    trip_freq_is_dense (mldsp_procs.hpp): general if some lane's frequency is positive and outside [2^-64, 2^64]; else trips if every
    lane's is inside (0, 1/16]; else fast."""
    f = np.asarray(freq, np.float32).reshape(-1, 64)
    odd = (f > 0) & ~((f >= np.float32(2.0 ** -64)) & (f <= np.float32(2.0 ** 64)))
    dense = ~((f > 0) & (f <= np.float32(1.0 / 16.0)))
    return np.where(odd.any(1), "general", np.where(dense.any(1), "fast", "trip"))


@functools.lru_cache(maxsize=None)
def expected(head, T):
    """The checker's outputs [V][64 T] of CALLS consecutive launches and the state after them: once per head and T, never written."""
    from cpu_checkers import Oracle
    orc = Oracle()
    st = orc.chain_clear(SAW_BP_GAIN, V)
    outs = [orc.chain_process(SAW_BP_GAIN, T, bank_coeffs(), st, None, frequencies(head), n_threads=4) for _ in range(CALLS)]
    for o in outs:
        o.setflags(write=False)
    st.setflags(write=False)
    return outs, st


@pytest.fixture(scope="module")
def engines():
    import madronalib_amd as ml
    es = {}
    for mode in MODES:
        es[mode] = ml.Engine(0)
        es[mode].set_launch_parts(mode)
    es[1].mixdown_reserve(V, 1)
    yield es
    for e in es.values():
        e.close()


def make_bank(eng, head):
    bank = eng.bank(SAW_BP_GAIN, V)
    assert bank.fused and bank.kernel_name.startswith("chain_kernel<mldev::Chain<2")
    bank.clear()
    bank.set_all_coeffs(bank_coeffs())
    bank.set_input_const(frequencies(head))
    return bank


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("head", HEADS)
def test_bank_in_one_two_and_four_kernels(engines, head, T):
    want, want_state = expected(head, T)
    assert np.isfinite(want[-1]).all() and np.abs(want[-1]).max() > 1e-3
    got = {}
    for mode in MODES:
        eng = engines[mode]
        split = eng.launch_stats()[0]
        bank = make_bank(eng, head)
        outs = [bank.process_host(T, None, Layout.QUAD) for _ in range(CALLS)]
        got[mode] = (outs, bank.get_all_state())
        bank.close()
        assert eng.launch_stats()[0] - split == (0 if mode == 1 else CALLS), f"parts = {mode}"
        label = f"{head} head, T = {T}, parts = {mode}: "
        for k in range(CALLS):
            assert_bits_equal(outs[k], want[k], True, label + f"launch {k} against the checker")
            assert_bits_equal(outs[k], got[1][0][k], True, label + f"launch {k} against one kernel")
        assert_bits_equal(got[mode][1], want_state, False, label + "final state against the checker")
        assert_bits_equal(got[mode][1], got[1][1], False, label + "final state against one kernel")


@pytest.mark.parametrize("head", HEADS)
def test_bank_mix_form(engines, oracle, head):
    """The same bank through chain_mix_kernel, T = 1: the voices' sum and the final state."""
    T = 1
    (y, _), _ = expected(head, T)
    st = oracle.chain_clear(SAW_BP_GAIN, V)
    assert_bits_equal(oracle.chain_process(SAW_BP_GAIN, T, bank_coeffs(), st, None, frequencies(head), n_threads=4), y, True, "the checker repeats itself")
    want = oracle.mixdown(y, None)
    eng = engines[1]
    bank = make_bank(eng, head)
    d_out = eng.alloc(4 * 64 * T)
    bank.process_mixdown(T, d_out, None, Layout.QUAD, None)
    got, gst = d_out.download(np.float32, 64 * T), bank.get_all_state()
    bank.close()
    assert np.isfinite(want).all() and np.abs(want).max() > 1e-6
    assert_bits_equal(got, want, True, f"mix form, {head} head")
    assert_bits_equal(gst, st, False, "final state")


def test_cascade(engines, oracle):
    """cascade_lanes_kernel's turn point, once per DSPVector: Lopass x 8 over 4 096 channels of a streamed input, T = 2, two launches."""
    procs, Vc, T = [Proc.LOPASS] * 8, 4096, 2
    co = chain_coeffs(oracle, procs, Vc, seed=3)
    sig, const = chain_input(procs, Vc, CALLS * T, seed=8)
    assert sig is not None and const is None
    st = oracle.chain_clear(procs, Vc)
    eng = engines[1]
    bank = eng.bank(procs, Vc)
    assert bank.fused and "cascade" in bank.kernel_name
    bank.set_all_coeffs(co)
    bank.set_all_state(st.copy())
    for k in range(CALLS):
        x = np.ascontiguousarray(sig[:, 64 * T * k:64 * T * (k + 1)])
        got = bank.process_host(T, x, Layout.QUAD)
        want = oracle.chain_process(procs, T, co, st, x, None, n_threads=4)
        assert_bits_equal(got, want, True, f"cascade launch {k}")
        assert np.abs(want).max() > 1e-6
    assert_bits_equal(bank.get_all_state(), st, False, "cascade final state")
    bank.close()


@pytest.mark.parametrize("vpl", [1, 2])
def test_graph_kernel(engines, oracle, vpl):
    """A generated graph kernel's turn points (every two quads): patches.synth16() at 2 048 voices, T = 2, two launches, every output
    word and every state word against the graph oracle."""
    Vg, T = 2048, 2
    eng = engines[1]
    params, coeffs = synth16_setup(oracle, Vg, seed=12)
    seeds = np.arange(Vg, dtype=np.uint32) * np.uint32(2654435761)
    g, desc, outs, states = build_synth16(eng, oracle, Vg, params, coeffs, seeds, vpl)
    assert f"({vpl} voice" in g.source
    gate = gate_signal(Vg, 64 * T * CALLS, seed=13)
    gate[:, :40] = np.float32(0.8)     # (every voice sounds from the first launch on)
    for call in range(CALLS):
        sig = {"gate": np.ascontiguousarray(gate[:, call * 64 * T:(call + 1) * 64 * T])}
        (got,) = g.process_host(T, sig, Layout.QUAD)
        (want,) = evaluate(oracle, desc, outs, Vg, T, sig, params, coeffs, states)
        assert_bits_equal(got, want, True, f"synth16, {vpl} voice(s) per lane, launch {call}")
    for n in desc:
        if n["type"] == "proc":
            for i in range(g.num_state(n["name"])):
                assert (g.get_state(n["name"], i) == states[n["name"]][i]).all(), (n["name"], i)
    assert 2 * np.count_nonzero(want) >= want.size
    g.close()
