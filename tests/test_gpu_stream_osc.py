"""GPU parity of the SawGen / PulseGen pair on a streamed frequency - every branch of GraphEmitter::streamLockPair, every exit of
step_locked_stream<true / false>, next_sw with oddW both ways, next2 - and of the [SAW_GEN] / [PULSE_GEN] banks on the same signal,
against the oracle, bit for bit (any NaN equals any NaN), with every oscillator's final counter. The cases and their roles:
tests/stream_osc_cases.py; that they do reach every class: tests/test_stream_osc_cpu.py's census."""
import time

import numpy as np
import pytest

import stream_osc_cases as sc
from graph_oracle import evaluate, evaluate_stream, new_stream_state
from inputs import assert_bits_equal
from madronalib_amd.constants import Layout, Proc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import madronalib_amd as ml
    e = ml.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data():
    return sc.census_data()


@pytest.fixture(scope="module")
def cases(data):
    return sc.all_graph_cases(data)


def run_launch(eng, g, case, T, sig, layout):
    """Graph.process_host, except that a mixed-down output is 64 T floats in no layout: -> list of [V][64 T] (plain) / [64 T] (mixed)."""
    V = case.V
    nbytes = V * T * 64 * 4
    d_in = []
    for name in g.inputs:
        d = eng.to_device(np.ascontiguousarray(sig[name], np.float32))
        if layout != Layout.VOICE_MAJOR:
            q = eng.alloc(nbytes)
            eng.layout_convert(d, Layout.VOICE_MAJOR, q, layout, V, T)
            d = q
        d_in.append(d)
    d_out = [eng.alloc(4 * 64 * T if i in case.mix else nbytes) for i in range(len(case.outs))]
    g.process(T, d_in, d_out, layout, layout)
    res = []
    for i, d in enumerate(d_out):
        if i in case.mix:
            res.append(d.download(np.float32, 64 * T).copy())
            continue
        if layout != Layout.VOICE_MAJOR:
            r = eng.alloc(nbytes)
            eng.layout_convert(d, layout, r, Layout.VOICE_MAJOR, V, T)
            d = r
        res.append(d.download(np.float32, V * T * 64).reshape(V, 64 * T).copy())
    return res


@pytest.mark.parametrize("name", sc.STRUCTURAL + sc.LOCKS)
def test_stream_pair_vs_oracle(eng, oracle, cases, name):
    import madronalib_amd as ml
    t0 = time.perf_counter()
    case = cases[name]
    V = case.V
    g = ml.Graph(eng, V, case.desc, case.outs, compile_now=False, **case.kwargs)
    for o in case.mix:
        g.set_output_mixdown(o)
    g.compile()
    sc.assert_forms(case, g.source)
    g.clear()
    if case.mix:
        g.reserve_mixdown(max(t for t, _ in case.launches))
    for k, v in case.params.items():
        g.set_param(k, v)
    for k, c in case.coeffs.items():
        g.set_coeffs(k, [np.ascontiguousarray(r) for r in c])
    stream = any(d["type"] == "proc" and d["kind"] in Proc.DELAYS for d in case.desc)
    if stream:
        states = new_stream_state(oracle, case.desc, V)
    else:
        states = {d["name"]: oracle.chain_clear([d["kind"]], V) for d in case.desc if d["type"] == "proc"}
    for o, ph in case.start_states.items():
        g.set_state(o, 0, ph)
        states[o][0] = ph
    at, got_saw = 0, []
    for call, (T, edit) in enumerate(case.launches):
        if edit is not None:
            new = sc.apply_launch_edit(edit, g.get_state("saw", 0), g.get_state("pulse", 0))
            g.set_state("pulse", 0, new)
            states["pulse"][0] = new
        sig = {k: np.ascontiguousarray(x[:, at:at + 64 * T]) for k, x in case.input_signals.items()}
        at += 64 * T
        got = run_launch(eng, g, case, T, sig, Layout.QUAD if call == 0 else Layout.VOICE_MAJOR)
        want = (evaluate_stream if stream else evaluate)(oracle, case.desc, case.outs, V, T, sig, case.params, case.coeffs, states)
        for i, o in enumerate(case.outs):
            w = oracle.mixdown(want[i]) if i in case.mix else want[i]
            assert_bits_equal(got[i], w, True, f"{name}: output {o} launch {call}")
        got_saw.append(got[case.outs.index("saw")])
        # after EVERY launch, before the next one's edit: a wavefront that ran locked where it should have fallen back has made the
        # pulse's counter the saw's
        for o in case.start_states:
            assert (g.get_state(o, 0) == states[o][0]).all(), f"{name}: counter of {o} after launch {call}"
    g.close()
    # the corrections did happen: next to a step the saw differs from the naive 2 p - 1 (p: the oracle's PhasorGen on the same frequency)
    st = np.ascontiguousarray(case.start_states["saw"][None, :].copy())
    p = oracle.chain_process([Proc.PHASOR_GEN], at // 64, np.zeros((0, V), np.float32), st, sc.freq_of(oracle, case), None)
    with np.errstate(invalid="ignore"):
        differs = np.abs(np.concatenate(got_saw, 1).astype(np.float64) - (2.0 * p.astype(np.float64) - 1.0)) > 1e-3
    assert differs[case.loud].mean() > 0.005, (name, differs[case.loud].mean())
    print(f"{name}: V {V}, {at // 64} DSPVectors, corrected share of the loud voices' samples {differs[case.loud].mean():.4f}, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("kind", [Proc.SAW_GEN, Proc.PULSE_GEN])
def test_stream_banks_vs_oracle(eng, oracle, data, kind):
    """chain_kernel<Chain<kind>, HAS_SIGNAL> on the census's signal: a frequency that moves every sample, quiet wavefronts (the SKIP
    exit), lanes inside two zones, hostile frequencies, absurd widths as the PulseGen's coefficient; two launches with carried state."""
    t0 = time.perf_counter()
    procs, co, st, sig = sc.bank_case(data, kind)
    V, T = sc.V0, sc.T0
    bank = eng.bank(procs, V)
    bank.set_all_coeffs(co)
    bank.set_all_state(st.copy())
    for call, layout in enumerate((Layout.QUAD, Layout.VOICE_MAJOR)):
        part = np.ascontiguousarray(sig[:, call * 64 * T:(call + 1) * 64 * T])
        got = bank.process_host(T, part, layout)
        want = oracle.chain_process(procs, T, co, st, part, None, n_threads=4)
        assert_bits_equal(got, want, True, f"bank of kind {kind} launch {call}")
        assert_bits_equal(bank.get_all_state(), st, False, f"bank of kind {kind}: counters after launch {call}")
        if kind == Proc.SAW_GEN and call == 0:
            first = got
    bank.close()
    if kind == Proc.SAW_GEN:
        st = np.ascontiguousarray(data["phases"][None, :].copy())
        p = oracle.chain_process([Proc.PHASOR_GEN], T, np.zeros((0, V), np.float32), st, np.ascontiguousarray(sig[:, :64 * T]), None)
        with np.errstate(invalid="ignore"):
            differs = np.abs(first.astype(np.float64) - (2.0 * p.astype(np.float64) - 1.0)) > 1e-3
        assert differs[sc.wave_of() >= 16].mean() > 0.005
    print(f"bank {kind}: {time.perf_counter() - t0:.2f} s")
