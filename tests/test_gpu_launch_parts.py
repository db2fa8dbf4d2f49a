"""Launches in two parts (mlgpu_engine_set_launch_parts; DESIGN.md §3.1, "Launch parts"): a plain launch of a bank going out as two
kernels on two streams computes the bits one launch computes, the streams meet again before anything else the engine does, and no
other form ever goes out in parts. T = 3; config 3's chain (ahead of time) and SineGen -> Lopass -> Gain (generated)."""
import functools

import numpy as np
import pytest

from inputs import assert_bits_equal
from madronalib_amd.constants import Layout, Op, Proc

pytestmark = pytest.mark.gpu

T = 3
UNIT = 2048                      # mlparts::kSplitUnit: 8 workgroups of 256 lanes
CHAINS = {"saw": [Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN], "sine": [Proc.SINE_GEN, Proc.LOPASS, Proc.GAIN]}
SHAPES = [2304, 4096, 256]       # a ragged second part (2048 + 256), two whole units, one workgroup (never in parts)


@functools.lru_cache(maxsize=None)
def voice_params(chain, V):
    """(freq [V], coeffs [4][V]): per-voice frequencies 55 Hz .. 1.76 kHz at 48 kHz and filter coefficients from a palette of 64."""
    import madronalib_amd as ml
    make = ml.Bandpass.makeCoeffs if chain == "saw" else ml.Lopass.makeCoeffs
    freq = (55.0 * 2.0 ** (5.0 * ((np.arange(V) * 37) % V) / V) / 48000.0).astype(np.float32)
    palette = np.stack([make(0.01 + 0.4 * j / 64, 0.3 + 0.5 * (j % 7) / 7) for j in range(64)], 1).astype(np.float32)   # [3][64]
    gain = (0.125 + 0.5 * (np.arange(V) % 5) / 5).astype(np.float32)
    return freq, np.ascontiguousarray(np.concatenate([palette[:, (np.arange(V) * 13) % 64], gain[None]], 0))


@functools.lru_cache(maxsize=None)
def expected(chain, V, calls=3):
    """The CPU checker's outputs [V][64 T] of `calls` consecutive process calls and the state after them: computed once, never written."""
    from cpu_checkers import Oracle
    orc = Oracle()
    freq, coeffs = voice_params(chain, V)
    st = orc.chain_clear(CHAINS[chain], V)
    outs = [orc.chain_process(CHAINS[chain], T, coeffs, st, None, freq, n_threads=4) for _ in range(calls)]
    for o in outs:
        o.setflags(write=False)
    st.setflags(write=False)
    return outs, st


def make_bank(eng, chain, V):
    freq, coeffs = voice_params(chain, V)
    bank = eng.bank(CHAINS[chain], V)
    assert bank.fused
    bank.clear()
    bank.set_all_coeffs(coeffs)
    bank.set_input_const(freq)
    return bank


def voice_major(raw, V, layout=Layout.QUAD):
    """A downloaded signal as [V][64 T]."""
    if layout == Layout.QUAD:
        return raw.reshape(T, 16, V, 4).transpose(2, 0, 1, 3).reshape(V, 64 * T)
    if layout == Layout.ROWS:
        return raw.reshape(T, V, 64).transpose(1, 0, 2).reshape(V, 64 * T)
    return raw.reshape(V, 64 * T)


def joins_during(eng, work):
    before = eng.launch_stats()[1]
    work()
    return eng.launch_stats()[1] - before


@pytest.fixture()
def engine():
    """A fresh engine per test (the counters start at zero), parts = 2: in two parts whenever the form allows."""
    import madronalib_amd as ml
    e = ml.Engine(0)
    e.set_launch_parts(2)
    assert e.get_launch_parts() == 2
    yield e
    e.close()


@pytest.fixture()
def plain():
    """... and the yardstick: parts = 1, always one launch."""
    import madronalib_amd as ml
    e = ml.Engine(0)
    e.set_launch_parts(1)
    yield e
    e.close()


# ---- in two parts == in one == the CPU checker ----
@pytest.mark.parametrize("V", SHAPES)
@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_parts_equal_one_launch_equal_the_checker(engine, plain, chain, V):
    """Three consecutive process calls into two alternating buffers: the outputs still there afterwards (calls 1 and 2) and the
    state, in two parts and in one, are the checker's bits. Between the calls the streams never meet."""
    want, want_state = expected(chain, V)
    n = V * T * 64
    for eng in (engine, plain):
        bank = make_bank(eng, chain, V)
        bufs = [eng.alloc(4 * n), eng.alloc(4 * n)]
        eng.sync()
        assert joins_during(eng, lambda: [bank.process(T, bufs[k & 1], Layout.QUAD) for k in range(3)]) == 0
        split, _ = eng.launch_stats()
        assert split == (3 if eng is engine and V > UNIT else 0), f"launches in two parts at V = {V}"
        label = f"{chain}, V = {V}, parts = {eng.get_launch_parts()}"
        assert_bits_equal(voice_major(bufs[1].download(), V), want[1], what=label + ": the second call's output")
        assert_bits_equal(voice_major(bufs[0].download(), V), want[2], what=label + ": the third call's output")
        assert (bank.get_all_state() == want_state).all(), label + ": the state read back"
        assert eng.launch_stats()[1] == (1 if eng is engine and V > UNIT else 0)   # the first download met the side stream, once


@pytest.mark.parametrize("layout", [Layout.ROWS, Layout.VOICE_MAJOR])
def test_parts_in_the_other_layouts(engine, layout):
    """The second part's output starts at its first voice in every layout (V = 2304: voices 2048 .. 2303)."""
    V = 2304
    want, _ = expected("saw", V)
    bank = make_bank(engine, "saw", V)
    d_out = engine.alloc(4 * V * T * 64)
    bank.process(T, d_out, layout)
    assert engine.launch_stats()[0] == 1
    assert_bits_equal(voice_major(d_out.download(), V, layout), want[0], what=f"layout {int(layout)}")


# ---- the join rule ----
V_RULE = 2304


def test_update_between_two_calls(engine, plain):
    """process, a full-row set_coeff and a stream-ordered sparse update, process: the updates wait for both parts of the first call and
    the second call sees them in both parts."""
    import madronalib_amd as ml
    n = V_RULE * T * 64
    got = {}
    for eng in (engine, plain):
        bank = make_bank(eng, "saw", V_RULE)
        d_out = [eng.alloc(4 * n), eng.alloc(4 * n)]
        bank.process(T, d_out[0], Layout.QUAD)
        j = joins_during(eng, lambda: bank.set_coeff(2, 0, np.linspace(0.1, 0.9, V_RULE, dtype=np.float32)))
        bank.process(T, d_out[1], Layout.QUAD)
        j2 = joins_during(eng, lambda: bank.apply_updates([ml.Update.coeff(2, 0, 100, 2150, 0.5), ml.Update.input_const(2040, 20, 0.01)]))
        bank.process(T, d_out[0], Layout.QUAD)
        got[eng] = (j, j2, d_out[1].download(), d_out[0].download(), bank.get_all_state())
    assert got[engine][:2] == (1, 1) and got[plain][:2] == (0, 0)
    assert engine.launch_stats()[0] == 3
    for k, what in ((2, "after set_coeff"), (3, "after apply_updates")):
        assert_bits_equal(got[engine][k], got[plain][k], what=what)
    assert np.array_equal(got[engine][4], got[plain][4]), "state"


def test_read_back_after_one_call(engine):
    want, _ = expected("saw", V_RULE)
    bank = make_bank(engine, "saw", V_RULE)
    d_out = engine.alloc(4 * V_RULE * T * 64)
    bank.process(T, d_out, Layout.QUAD)
    assert engine.launch_stats() == (1, 0)
    assert_bits_equal(voice_major(d_out.download(), V_RULE), want[0], what="the first call's output")
    assert engine.launch_stats() == (1, 1)


def test_same_buffer_twice_needs_no_join(engine):
    want, _ = expected("saw", V_RULE)
    bank = make_bank(engine, "saw", V_RULE)
    d_out = engine.alloc(4 * V_RULE * T * 64)
    bank.process(T, d_out, Layout.QUAD)
    assert joins_during(engine, lambda: bank.process(T, d_out, Layout.QUAD)) == 0
    assert engine.launch_stats() == (2, 0)
    assert_bits_equal(voice_major(d_out.download(), V_RULE), want[1], what="the second call's output")


def test_overlapping_buffer_at_another_base_joins(engine, plain):
    """The second call's output overlaps the first's 64 KiB further on: its first part would write where the first call's second part
    may still be writing. Also: the same base in another layout, and over another length."""
    n = V_RULE * T * 64
    got = {}
    for eng in (engine, plain):
        bank = make_bank(eng, "saw", V_RULE)
        big = eng.alloc(4 * n + 65536)
        bank.process(T, big, Layout.QUAD)
        j = [joins_during(eng, lambda: bank.process(T, big.ptr + 65536, Layout.QUAD)),
             joins_during(eng, lambda: bank.process(T, big.ptr + 65536, Layout.ROWS)),
             joins_during(eng, lambda: bank.process(T - 1, big.ptr + 65536, Layout.ROWS)),
             joins_during(eng, lambda: bank.process(T - 1, big.ptr + 65536, Layout.ROWS))]
        got[eng] = (j, big.download(), bank.get_all_state())
    assert got[engine][0] == [1, 1, 1, 0] and got[plain][0] == [0, 0, 0, 0]
    assert engine.launch_stats()[0] == 5
    assert_bits_equal(got[engine][1], got[plain][1], what="the buffer after the overlapping calls")
    assert np.array_equal(got[engine][2], got[plain][2]), "state"


def test_a_bank_that_streams_the_output_in_sees_all_of_it(engine, plain):
    """Bank X in two parts, then bank Y with X's output as its streamed input: Y goes out in one launch, after both parts of X."""
    import madronalib_amd as ml
    n = V_RULE * T * 64
    got = {}
    for eng in (engine, plain):
        x = make_bank(eng, "saw", V_RULE)
        y = eng.bank([Proc.LOPASS, Proc.GAIN], V_RULE)
        y.set_coeffs(0, ml.Lopass.makeCoeffs(0.05, 0.7))
        y.set_coeff(1, 0, 0.5)
        d_x, d_y = eng.alloc(4 * n), eng.alloc(4 * n)
        x.process(T, d_x, Layout.QUAD)
        j = joins_during(eng, lambda: y.process(T, d_y, Layout.QUAD, d_x, Layout.QUAD))
        got[eng] = (j, eng.launch_stats()[0], d_y.download())
    assert got[engine][:2] == (1, 1) and got[plain][:2] == (0, 0)
    assert_bits_equal(got[engine][2], got[plain][2], what="the streaming bank's output")
    # (and X's own output is the checker's)
    assert_bits_equal(voice_major(d_x.download(), V_RULE), expected("saw", V_RULE)[0][0], what="bank X")


@pytest.mark.parametrize("how", ["sync", "timer_stop", "fence"])
def test_waiting_sees_both_parts_done(engine, plain, how):
    """After engine.sync(), after timer_stop_ms(), and behind a fence another engine waits for, both parts are done: the output, read
    through ANOTHER engine's stream (which has no order of its own with the side stream), is complete."""
    want, _ = expected("saw", V_RULE)
    bank = make_bank(engine, "saw", V_RULE)
    d_out = engine.alloc(4 * V_RULE * T * 64)
    engine.sync()
    if how == "timer_stop":
        engine.timer_start()
    bank.process(T, d_out, Layout.QUAD)
    assert engine.launch_stats() == (1, 0)
    if how == "sync":
        engine.sync()
    elif how == "timer_stop":
        assert engine.timer_stop_ms() > 0.0
    else:
        f = engine.fence()
        engine.signal(f)
        plain.wait(f)
    assert engine.launch_stats() == (1, 1)
    raw = np.empty(V_RULE * T * 64, np.float32)
    plain._check(plain.L.mlgpu_download(plain.h, raw.ctypes.data, d_out.ptr, raw.nbytes))
    assert_bits_equal(voice_major(raw, V_RULE), want[0], what=how)
    assert engine.launch_stats() == (1, 1)


def test_free_and_close_with_side_work_pending(engine):
    want, _ = expected("saw", V_RULE)
    n = V_RULE * T * 64
    bank = make_bank(engine, "saw", V_RULE)
    a, b = engine.alloc(4 * n), engine.alloc(4 * n)
    bank.process(T, a, Layout.QUAD)
    bank.process(T, b, Layout.QUAD)
    assert joins_during(engine, a.free) == 1       # freeing a buffer the side stream may be writing
    bank.process(T, b, Layout.QUAD)
    assert joins_during(engine, bank.close) == 1   # releasing the bank whose second part is in flight
    other = make_bank(engine, "saw", V_RULE)
    other.process(T, b, Layout.QUAD)
    assert engine.launch_stats()[0] == 4
    assert_bits_equal(voice_major(b.download(), V_RULE), want[0], what="a new bank after the old one was released")
    other.process(T, b, Layout.QUAD)
    # (the fixture closes the engine with the second part pending)


# ---- what never goes out in parts ----
def test_other_forms_never_go_out_in_parts(engine):
    import madronalib_amd as ml
    V = 4096
    n = V * T * 64
    bank = make_bank(engine, "saw", V)
    d_out, d_small = engine.alloc(4 * n), engine.alloc(4 * n)
    engine.mixdown_reserve(V, T)
    bank.process_mixdown(T, d_small)
    bank.process_groups(T, d_out, 4)
    bank.reserve_voice_list_groups(V, 4)
    bank.set_voice_list(np.arange(0, V, 3, dtype=np.uint32))
    bank.process_listed(T, d_out)
    bank.process_listed_groups(T, d_out)
    assert engine.launch_stats() == (0, 0), "mix, groups, listed, listed groups"
    # a streamed input
    flt = engine.bank([Proc.BANDPASS], V)
    flt.process(T, d_small, Layout.QUAD, d_out, Layout.QUAD)
    assert engine.launch_stats() == (0, 0), "a streamed-input bank"
    # a graph
    g = ml.Graph(engine, V, [dict(name="x", type="input"), dict(name="y", type="op", kind=Op.ADD, inputs=["x", "x"])], ["y"])
    g.process(T, [d_out], [d_small])
    assert engine.launch_stats() == (0, 0), "a graph"
    # a cascade on a launch-constant input
    casc = engine.bank([Proc.SAW_GEN] + [Proc.LOPASS] * 4, V)
    assert casc.kernel_name.startswith("cascade_")
    casc.set_input_const(voice_params("saw", V)[0])
    casc.process(T, d_out, Layout.QUAD)
    assert engine.launch_stats() == (0, 0), "a cascade"
    # anything while recording a sequence
    with engine.record() as seq:
        bank.process(T, d_out, Layout.QUAD)
    assert engine.launch_stats() == (0, 0), "while recording"
    seq.launch()
    engine.sync()
    assert engine.launch_stats() == (0, 0)
    # ... and the same call outside the recording does
    bank.process(T, d_out, Layout.QUAD)
    assert engine.launch_stats() == (1, 0)
    # recording a sequence meets the side stream first, and the launch inside it is one launch
    with engine.record() as seq2:
        bank.process(T, d_out, Layout.QUAD)
    assert engine.launch_stats() == (1, 1)
    seq2.launch()
    engine.sync()
    assert engine.launch_stats() == (1, 1)
    seq2.close()
    seq.close()


def test_an_engine_whose_stream_was_handed_out_stays_in_one_launch(engine):
    bank = make_bank(engine, "saw", 4096)
    d_out = engine.alloc(4 * 4096 * T * 64)
    assert engine.launch_parts_possible()
    assert engine.stream
    assert not engine.launch_parts_possible() and engine.get_launch_parts() == 2
    bank.process(T, d_out, Layout.QUAD)
    assert engine.launch_stats() == (0, 0)


def test_size_rule_of_the_default():
    """parts = 0: 4 096 voices stay in one launch; the headline's 262 144 voices go out in two parts (counted, not compared: the
    outputs are 200 MB)."""
    import madronalib_amd as ml
    eng = ml.Engine(0)
    try:
        assert eng.get_launch_parts() == 0
        small = make_bank(eng, "saw", 4096)
        d_small = eng.alloc(4 * 4096 * T * 64)
        small.process(T, d_small, Layout.QUAD)
        assert eng.launch_stats() == (0, 0)
        V = 262144
        big = eng.bank(CHAINS["saw"], V)
        big.clear()
        big.set_input_const(np.full(V, 440.0 / 48000.0, np.float32))
        d_big = [eng.alloc(4 * V * T * 64), eng.alloc(4 * V * T * 64)]
        for k in range(4):
            big.process(T, d_big[k & 1], Layout.QUAD)
        assert eng.launch_stats() == (4, 0)
        eng.sync()
        assert eng.launch_stats() == (4, 1)
    finally:
        eng.close()
