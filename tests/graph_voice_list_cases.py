"""Graphs, inputs and expected values of the graph voice-list calls (mlgpu_graph_set_voice_list, mlgpu_graph_process_listed), shared by
tests/test_graph_voice_list_cpu.py and tests/test_gpu_graph_voice_list.py.

The one rule: a listed call behaves as a graph of K voices with the same description, made of voices L[0] ... L[K-1]. For a graph
without rings the expected values are graph_oracle.evaluate on the K gathered voices - params, coefficients, input rows and control
columns gathered by L, the state taken from the full graph's state at L and scattered back there -, oracle.mixdown of those K rows and
the peaks in numpy. Ring memory cannot be read back from the device, so the ring cases of the voice-list tests take a plain K-voice graph
on the device as their expected value; the host reference for graphs with rings is tests/session_model.py (graph_oracle.evaluate_stream on
the gathered voices with per-voice ring memory), which tests/test_gpu_session_fuzz.py compares whole sessions with."""
import types

import numpy as np

from inputs import lcg_noise
from madronalib_amd.constants import Op, Proc, Region
from voice_list_cases import V, voice_lists

T = 3
LISTS = voice_lists()


# ---- the descriptions -------------------------------------------------------------------------------------------------------------
def synth_desc():
    """param freq -> SawGen and PulseGen (its width a coefficient) on the same freq - an oscillator trip pair; a streamed input; Lopass;
    one control; two outputs: the Lopass (plain) and Lopass * control (mixed down in the tests)."""
    return [dict(name="freq", type="param"),
            dict(name="saw", type="proc", kind=Proc.SAW_GEN, inputs=["freq"]),
            dict(name="pulse", type="proc", kind=Proc.PULSE_GEN, inputs=["freq"]),
            dict(name="x", type="input"),
            dict(name="osc", type="op", kind=Op.ADD, inputs=["saw", "pulse"]),
            dict(name="sum", type="op", kind=Op.ADD, inputs=["osc", "x"]),
            dict(name="lp", type="proc", kind=Proc.LOPASS, inputs=["sum"]),
            dict(name="amp", type="control"),
            dict(name="out", type="op", kind=Op.MULTIPLY, inputs=["lp", "amp"])], ["lp", "out"]


def string_desc():
    """A plucked string: input -> FractionalDelay with a per-voice delay time -> OnePole -> gain -> back in, one DSPVector late."""
    return [dict(name="x", type="input"), dict(name="dt", type="param"), dict(name="g", type="param"),
            dict(name="fb", type="feedback", source="loop"),
            dict(name="sum", type="op", kind=Op.ADD, inputs=["x", "fb"]),
            dict(name="line", type="proc", kind=Proc.FRACTIONAL_DELAY, inputs=["sum", "dt"], max_delay=180.0),
            dict(name="damp", type="proc", kind=Proc.ONE_POLE, inputs=["line"]),
            dict(name="loop", type="op", kind=Op.MULTIPLY, inputs=["damp", "g"])], ["line"]


def three_ring_desc():
    """Three delay nodes in series, each delay time per voice: with three rings ring layout 0 issues its reads early, by LDS-DMA."""
    return [dict(name="x", type="input"), dict(name="dt", type="param"), dict(name="dt2", type="param"), dict(name="g", type="param"),
            dict(name="fb", type="feedback", source="loop"),
            dict(name="sum", type="op", kind=Op.ADD, inputs=["x", "fb"]),
            dict(name="d1", type="proc", kind=Proc.INTEGER_DELAY, inputs=["sum", "dt"], max_delay=100.0),
            dict(name="d2", type="proc", kind=Proc.FRACTIONAL_DELAY, inputs=["d1", "dt2"], max_delay=180.0),
            dict(name="d3", type="proc", kind=Proc.INTEGER_DELAY, inputs=["d2", "dt"], max_delay=100.0),
            dict(name="loop", type="op", kind=Op.MULTIPLY, inputs=["d3", "g"])], ["d3", "d1"]


def gain_desc():
    return [dict(name="x", type="input"), dict(name="gain", type="proc", kind=Proc.GAIN, inputs=["x"])], ["gain"]


# ---- the cases: a description with everything that is per voice -----------------------------------------------------------------------
def irregular_voices():
    """(unequal, odd, dense): voices whose saw and pulse phase counters differ, whose pulse width is outside [0, 1], whose frequency is
    too high for a trip. Sparse - most wavefronts of the full graph hold none and take the fast paths - and placed so that BOTH
    wavefronts of the list k80 hold each of the first two kinds next to regular voices: one lane out of line after the gather."""
    L = LISTS["k80"].astype(np.int64)
    v = np.arange(V)
    unequal = np.union1d(v[v % 97 == 11], L[[5, 20, 70]])
    odd = np.union1d(v[v % 193 == 50], L[[9, 75]])
    dense = np.union1d(v[v % 211 == 100], L[[30]])
    return unequal, odd, dense


def synth_case(oracle, tiny=False):
    """The synth voice with per-voice frequencies, widths, filter coefficients and STATE (phases, filter memories) - nothing from
    clear. tiny: the control is in the 1e-39 range, so that the second output and its mixdown live among the denormals."""
    desc, outputs = synth_desc()
    rng = np.random.default_rng(4242)
    unequal, odd, dense = irregular_voices()
    freq = rng.uniform(0.001, 0.05, V).astype(np.float32)
    freq[dense] = np.float32(0.21)
    width = rng.uniform(0.1, 0.9, V).astype(np.float32)
    width[odd] = np.float32(1.5)
    import madronalib_amd as ml
    lp = np.stack([ml.Lopass.makeCoeffs(float(om), 0.7) for om in rng.uniform(0.02, 0.3, 16)], 1)[:, rng.integers(0, 16, V)]
    phase = rng.integers(0, 2 ** 32, V, dtype=np.uint64).astype(np.uint32)
    other = phase.copy()
    other[unequal] += np.uint32(0x12345678)
    states = {"saw": phase[None, :].copy(), "pulse": other[None, :].copy(),
              "lp": (rng.uniform(-0.2, 0.2, (2, V)).astype(np.float32)).view(np.uint32).copy()}
    for name, kind in (("saw", Proc.SAW_GEN), ("pulse", Proc.PULSE_GEN), ("lp", Proc.LOPASS)):
        assert states[name].shape == (oracle.num_state(kind), V)
    amp = rng.uniform(0.2, 1.0, (V, T)).astype(np.float32)
    if tiny:
        amp = (amp * np.float32(1e-39)).astype(np.float32)
    x = lcg_noise(np.arange(V, dtype=np.uint32) + 77, 64 * T) * np.float32(0.25)
    return types.SimpleNamespace(desc=desc, outputs=outputs, mix=(1,), inputs={"x": x}, groups={}, controls={"amp": amp}, params={"freq": freq},
                                 coeffs={"pulse": width[None, :].copy(), "lp": np.ascontiguousarray(lp, np.float32)}, states=states)


def ring_case(which):
    """The string / the three-ring graph, run from clear (ring memory cannot be set): per-voice delay times and gains, noise in."""
    desc, outputs = string_desc() if which == "string" else three_ring_desc()
    rng = np.random.default_rng(99 if which == "string" else 98)
    import madronalib_amd as ml
    params = {"dt": rng.uniform(1.0, 95.0, V).astype(np.float32), "g": rng.uniform(0.5, 0.95, V).astype(np.float32)}
    coeffs = {}
    if which == "string":
        coeffs["damp"] = np.stack([ml.OnePole.makeCoeffs(float(om)) for om in rng.uniform(0.05, 0.4, 16)], 1)[:, rng.integers(0, 16, V)].astype(np.float32)
    else:
        params["dt2"] = rng.uniform(1.0, 170.0, V).astype(np.float32)
    x = lcg_noise(np.arange(V, dtype=np.uint32) + 555, 64 * T)
    return types.SimpleNamespace(desc=desc, outputs=outputs, mix=(), inputs={"x": x}, groups={}, controls={}, params=params, coeffs=coeffs, states=None)


# ---- expected values ------------------------------------------------------------------------------------------------------------------
def gathered(case, L):
    """The case of the K voices L: every per-voice table gathered (states copied)."""
    L = np.asarray(L, np.int64)
    take = lambda d, axis: {k: np.ascontiguousarray(np.take(a, L, axis)) for k, a in d.items()}  # noqa: E731
    inputs = {k: np.ascontiguousarray(a[L // case.groups.get(k, 1)]) for k, a in case.inputs.items()}
    return types.SimpleNamespace(desc=case.desc, outputs=case.outputs, mix=case.mix, inputs=inputs, groups={}, controls=take(case.controls, 0),
                                 params=take(case.params, 0), coeffs=take(case.coeffs, 1), states=None if case.states is None else take(case.states, 1))


def expected_listed(oracle, case, L, states, t0=0, n=T, flush=False):
    """The oracle on the K listed voices for DSPVectors [t0, t0 + n): `states` {node: [NS][V]} (the full graph's) is read at L and
    updated at L in place. Returns the outputs' signals, [K][64 n] each (before any mixdown)."""
    import graph_oracle
    L = np.asarray(L, np.int64)
    if L.size == 0:
        return [np.zeros((0, 64 * n), np.float32) for _ in case.outputs]
    k = gathered(case, L)
    sig = {name: np.ascontiguousarray(a[:, 64 * t0:64 * (t0 + n)]) for name, a in k.inputs.items()}
    sig.update({name: np.ascontiguousarray(a[:, t0:t0 + n]) for name, a in k.controls.items()})
    st = {name: np.ascontiguousarray(a[:, L]) for name, a in states.items()}
    with oracle.flush_denormals(flush):
        ys = graph_oracle.evaluate(oracle, case.desc, case.outputs, L.size, n, sig, k.params, k.coeffs, st)
    for name in states:
        states[name][:, L] = st[name]
    return [np.ascontiguousarray(y, np.float32) for y in ys]


def expected_peaks(ys):
    """The outputs' signals [K][S] -> [K] uint32: the largest bits(y) & 0x7fffffff over every sample of every output."""
    bits = np.concatenate([np.ascontiguousarray(y, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF) for y in ys], 1)
    return bits.max(axis=1).astype(np.uint32) if bits.shape[1] else np.zeros(bits.shape[0], np.uint32)


def expected_mixdown(oracle, y, flush=False):
    if y.shape[0] == 0:
        return np.zeros(y.shape[1], np.float32)
    with oracle.flush_denormals(flush):
        return oracle.mixdown(y, None)


# ---- building a graph of a case ---------------------------------------------------------------------------------------------------------
def build_graph(engine, case, n_voices=V, voice_lists=True, delay_windows=False, compile_now=True):
    """The case's graph over n_voices voices (not yet loaded with the case's tables: see load_tables)."""
    import madronalib_amd as ml
    g = ml.Graph(engine, n_voices, case.desc, case.outputs, delay_windows=delay_windows, compile_now=False, voice_lists=voice_lists,
                 input_groups={list(case.inputs).index(k): p for k, p in case.groups.items()})
    for o in case.mix:
        g.set_output_mixdown(o, True)
    if compile_now and engine.h is not None:
        g.compile()
    return g


def load_tables(g, case):
    """clear(), then the case's params, coefficients and (if it has any) state words."""
    g.clear()
    for name, p in case.params.items():
        g.set_param(name, p)
    for name, co in case.coeffs.items():
        for i in range(co.shape[0]):
            g.set_coeff(name, i, np.ascontiguousarray(co[i]))
    for name, st in (case.states or {}).items():
        for i in range(st.shape[0]):
            g.set_state(name, i, st[i])


def upsample_graph(engine, n_voices, voice_lists=True, kind=Region.UPSAMPLE_2X):
    """fn = Lopass at twice the rate (an UPSAMPLE_2X region; DOWNSAMPLE_2X for the refusal) around a streamed input, then a Gain."""
    import madronalib_amd as ml
    g = ml.Graph(engine, n_voices)
    if voice_lists:
        g.enable_voice_lists()
    g.add("x", "input")
    g.begin_region(kind, ["x"], ["rx"])
    g.add("rlp", "proc", Proc.LOPASS, ["rx"])
    g.end_region("rlp", "ry")
    g.add("gain", "proc", Proc.GAIN, ["ry"])
    g.add_output("gain")
    return g
