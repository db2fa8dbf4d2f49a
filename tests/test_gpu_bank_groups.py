"""mlgpu_bank_process_groups (chain_group_kernel): a fused bank whose voices come in groups of adjacent voices - an input row per
in_group voices, an output channel per out_group voices, their sum in voice order made inside the voice kernel.

Expected values: the per-voice signals of the CPU checker (the oracle's chain_process, as in the bank parity tests), times the gain in
float32 where gains are given, added in voice order from +0 with float32 adds (bank_groups_cases.expected_group_sums; the checker's
flush mode where the engine flushes denormals). Every case is also compared with Bank.process -> multiply -> Engine.mixdown_groups on
the device: that comparison is HIP against HIP, one step removed from the oracle."""
import os
import subprocess

import numpy as np
import pytest

from bank_groups_cases import T, VOICES, Chain, expected_group_sums, special_gains
from inputs import assert_bits_equal
from madronalib_amd.constants import Layout, Op, Proc, Status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = np.uint32(0x7FC5A5A5)   # what the memory around an output holds before a launch
_oracle_cache = {}


@pytest.fixture(scope="module")
def eng():
    import madronalib_amd as ml
    e = ml.Engine(0)
    yield e
    e.set_flush_denormals(False)
    e.close()


def reference(oracle, name, V, in_group, flush):
    """(chain, its per-voice signals [V][64 T] and final state from the oracle), computed once per case and left unchanged."""
    key = (name, V, in_group, flush)
    if key not in _oracle_cache:
        ch = Chain(name, oracle, V, in_group)
        y, st = ch.oracle_voices(oracle, flush)
        y.setflags(write=False), st.setflags(write=False)
        _oracle_cache[key] = (ch, y, st)
    return _oracle_cache[key]


def make_bank(eng, ch):
    bank = eng.bank(ch.procs, ch.V)
    bank.clear()
    bank.set_all_coeffs(ch.coeffs)
    if ch.in_const is not None:
        bank.set_input_const(ch.in_const)
    return bank


def to_layout(eng, rows, layout, vectors):
    """[R][64 vectors] numpy -> a device signal of R rows in `layout`."""
    rows = np.ascontiguousarray(rows, np.float32)
    d = eng.to_device(rows)
    if layout == Layout.VOICE_MAJOR:
        return d
    d2 = eng.alloc(rows.nbytes)
    eng.layout_convert(d, Layout.VOICE_MAJOR, d2, layout, rows.shape[0], vectors)
    return d2


def run_groups(eng, bank, ch, out_group, splits, out_layout=Layout.QUAD, in_layout=Layout.QUAD, d_gains=None):
    """process_groups over launches of `splits` DSPVectors, each into an output with one guard channel's worth of memory behind it
    that must come back untouched. Returns [V / out_group][64 T]."""
    C, outs, t0 = ch.V // out_group, [], 0
    for n in splits:
        d_in = None if ch.in_rows is None else to_layout(eng, ch.in_rows[:, 64 * t0:64 * (t0 + n)], in_layout, n)
        d_out = eng.alloc(4 * (C + 1) * 64 * n)
        d_out.upload(np.full((C + 1) * 64 * n, GUARD, np.uint32))
        bank.process_groups(n, d_out, out_group, out_layout, d_in, in_layout, ch.in_group, d_gains)
        raw = d_out.download(np.uint32)
        assert (raw[C * 64 * n:] == GUARD).all(), "a channel past V / out_group was written (a dead group's store)"
        d_vm = eng.alloc(4 * C * 64 * n)
        eng.layout_convert(d_out, out_layout, d_vm, Layout.VOICE_MAJOR, C, n)
        outs.append(d_vm.download(np.float32, C * 64 * n).reshape(C, 64 * n))
        t0 += n
    return np.concatenate(outs, 1)


def two_step(eng, ch, out_group, d_gains=None):
    """The route this call replaces, on the device: Bank.process on the input expanded to V rows, the gains as an elementwise
    multiply, Engine.mixdown_groups (out_group 1: the scaled voices themselves). Returns ([V / out_group][64 T], the bank's state)."""
    V, n = ch.V, V_floats(ch.V)
    bank = make_bank(eng, ch)
    d_in = None if ch.in_rows is None else eng.to_device(np.ascontiguousarray(np.repeat(ch.in_rows, ch.in_group, axis=0)))
    d_v = eng.alloc(4 * n)
    bank.process(T, d_v, Layout.VOICE_MAJOR, d_in, Layout.VOICE_MAJOR)
    if d_gains is not None:
        g = d_gains.download(np.float32, V)
        d_g = eng.to_device(np.ascontiguousarray(np.repeat(g[:, None], 64 * T, axis=1)))
        d_s = eng.alloc(4 * n)
        eng.op_apply(Op.MULTIPLY, d_v, d_g, None, d_s, n)
        d_v = d_s
    if out_group > 1:
        d_o = eng.alloc(4 * n // out_group)
        eng.mixdown_groups(d_v, Layout.VOICE_MAJOR, V // out_group, out_group, T, d_o, Layout.VOICE_MAJOR)
        d_v = d_o
    out = d_v.download(np.float32, n // out_group).reshape(V // out_group, 64 * T)
    st = bank.get_all_state()
    bank.close()
    return out, st


def V_floats(V):
    return V * 64 * T


def check_case(eng, oracle, name, V, in_group, out_group, flush=False, gains=None, out_layout=Layout.QUAD, in_layout=Layout.QUAD):
    ch, y, st = reference(oracle, name, V, in_group, flush)
    want = expected_group_sums(oracle, y, out_group, gains, flush)
    what = f"{name} V={V} in={in_group} out={out_group} flush={flush} gains={gains is not None}"
    eng.set_flush_denormals(flush)
    try:
        d_gains = None if gains is None else eng.to_device(gains)
        bank = make_bank(eng, ch)
        one = run_groups(eng, bank, ch, out_group, [T], out_layout, in_layout, d_gains)
        state_one = bank.get_all_state()
        bank.clear()
        split = run_groups(eng, bank, ch, out_group, [1, T - 1], out_layout, in_layout, d_gains)
        state_split = bank.get_all_state()
        bank.close()
        hip, state_process = two_step(eng, ch, out_group, d_gains)
    finally:
        eng.set_flush_denormals(False)
    assert np.isfinite(want).all() and np.abs(want).max() > 1e-6, what
    assert_bits_equal(one, want, True, what + ": one launch against the oracle")
    assert_bits_equal(split, one, True, what + ": launches of 1 + 2 against one launch")
    assert_bits_equal(one, hip, True, what + ": against process -> multiply -> mixdown_groups (HIP against HIP)")
    assert_bits_equal(state_one, st, False, what + ": state against the oracle")
    assert_bits_equal(state_split, state_process, False, what + ": state after 1 + 2 against mlgpu_bank_process's")
    assert_bits_equal(state_one, state_process, False, what + ": state against mlgpu_bank_process's")


CONST_CASES = [("saw", 2), ("saw", 4), ("saw", 8), ("saw", 16), ("saw_odd", 4), ("saw_odd", 16),
               ("impulse", 2), ("impulse", 4), ("impulse", 8), ("impulse", 16)]
SIGNAL_CASES = [(2, 2), (4, 4), (8, 8), (16, 16), (16, 4), (1, 16), (8, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("V", VOICES)
@pytest.mark.parametrize("name,out_group", CONST_CASES)
def test_group_sums_of_a_bank_on_its_constant_input(eng, oracle, name, out_group, V):
    """No streamed input: SawGen -> Bandpass -> Gain with the fast head (saw) and with one lane that sends its wavefront to the slow
    head (saw_odd), and ImpulseGen (its LDS table and workgroup barrier beside the strip). Output groups of 2, 4, 8 (lane shifts) and
    16 (the LDS strip); 80 voices (a quarter wavefront: dead lanes, dead groups) and 2 352 (eight remapped workgroups, one not, a
    last one of 48 voices). One launch of 3 DSPVectors, launches of 1 + 2, state against mlgpu_bank_process's, guard channel."""
    check_case(eng, oracle, name, V, 1, out_group)


@pytest.mark.gpu
@pytest.mark.parametrize("V", VOICES)
@pytest.mark.parametrize("in_group,out_group", SIGNAL_CASES)
def test_group_sums_of_a_filter_bank_on_shared_input_rows(eng, oracle, in_group, out_group, V):
    """Bandpass alone on a streamed input of V / in_group rows (HAS_SIGNAL, the input group): in_group == out_group of 2, 4, 8, 16, and
    the cross cases (in 16, out 4), (in 1, out 16), (in 8, out 1: the plain store)."""
    check_case(eng, oracle, "bandpass", V, in_group, out_group)


@pytest.mark.gpu
@pytest.mark.parametrize("V", VOICES)
@pytest.mark.parametrize("in_group,out_group,out_layout,in_layout", [(16, 16, Layout.VOICE_MAJOR, Layout.ROWS), (4, 4, Layout.VOICE_MAJOR, Layout.QUAD),
                                                                     (8, 1, Layout.QUAD, Layout.ROWS), (2, 8, Layout.VOICE_MAJOR, Layout.ROWS)])
def test_layouts_of_the_group_signals(eng, oracle, in_group, out_group, out_layout, in_layout, V):
    """The output in VOICE_MAJOR as well as QUAD, the input in ROWS as well as QUAD (the other tests run QUAD in, QUAD out)."""
    check_case(eng, oracle, "bandpass", V, in_group, out_group, out_layout=out_layout, in_layout=in_layout)


@pytest.mark.gpu
@pytest.mark.parametrize("flush", [pytest.param(False, id="ieee"), pytest.param(True, id="flush")])
@pytest.mark.parametrize("V", VOICES)
@pytest.mark.parametrize("name,in_group,out_group", [("saw", 1, 16), ("saw_odd", 1, 4), ("bandpass", 16, 16), ("bandpass", 8, 1), ("bandpass", 2, 2),
                                                     ("impulse", 1, 8)])
def test_per_voice_gains_in_both_float_modes(eng, oracle, name, in_group, out_group, V, flush):
    """Per-voice gains - a -0.0, a 0.0 and a denormal among them, in the first group and in the last - multiply each voice before the
    sum; with the engine honouring denormals and flushing them (the group adds obey the mode like every other add)."""
    check_case(eng, oracle, name, V, in_group, out_group, flush=flush, gains=special_gains(V))


@pytest.mark.gpu
@pytest.mark.parametrize("layout,in_layout", [(Layout.QUAD, None), (Layout.VOICE_MAJOR, Layout.ROWS), (Layout.ROWS, Layout.VOICE_MAJOR)])
def test_host_convenience_and_a_broadcast_input(eng, oracle, layout, in_layout):
    """Bank.process_groups_host (numpy in, numpy out, the layout conversions on the device) against the oracle, with an input group,
    gains and 80 voices; and one broadcast row for all voices (in_group 1) against the same row given per voice."""
    ch, y, _ = reference(oracle, "bandpass", 80, 8, False)
    gains = special_gains(ch.V)
    bank = make_bank(eng, ch)
    got = bank.process_groups_host(T, 4, in_signal=ch.in_rows, in_group=8, gains=gains, layout=layout, in_layout=in_layout)
    assert_bits_equal(got, expected_group_sums(oracle, y, 4, gains), True, "process_groups_host against the oracle")
    bank.clear()
    d_row = eng.to_device(np.ascontiguousarray(ch.in_rows[0]))           # BROADCAST: [64 T], one voice's stream
    d_out = eng.alloc(4 * (ch.V // 16) * 64 * T)
    bank.process_groups(T, d_out, 16, Layout.VOICE_MAJOR, d_row, Layout.BROADCAST, 1)
    one_row = d_out.download(np.float32).reshape(ch.V // 16, 64 * T)
    bank.clear()
    per_voice = bank.process_groups_host(T, 16, in_signal=np.repeat(ch.in_rows[:1], ch.V, axis=0), layout=layout, in_layout=in_layout)
    assert_bits_equal(one_row, per_voice, True, "a broadcast input against the same row per voice")
    assert np.abs(one_row).max() > 1e-6
    bank.close()


@pytest.mark.gpu
def test_refusals_leave_the_state_alone(eng, oracle):
    """A group of 3, voices that are not whole groups, an input group without an input, a null or misaligned output, a bad layout:
    MLGPU_ERR_INVALID; a cascade bank and a processor-by-processor bank: MLGPU_ERR_UNSUPPORTED, naming the two other routes. Each with
    a message, nothing launched: the state stays what it was."""
    import madronalib_amd as ml
    ch, _, _ = reference(oracle, "saw", 80, 1, False)
    bank = make_bank(eng, ch)
    d_out = eng.alloc(4 * 80 * 64)
    bank.process(1, d_out)           # (a state that is not the cleared one)
    before = bank.get_all_state()

    def refused(status, words, b, *args, **kw):
        with pytest.raises(ml.MlgpuError) as ei:
            b.process_groups(*args, **kw)
        assert ei.value.status == status, str(ei.value)
        assert all(w in str(ei.value) for w in words), str(ei.value)

    refused(Status.ERR_INVALID, ["bank_process_groups", "1, 2, 4, 8 or 16"], bank, 1, d_out, 3)
    refused(Status.ERR_INVALID, ["bank_process_groups", "1, 2, 4, 8 or 16"], bank, 1, d_out, 4, d_in=d_out, in_group=3)
    refused(Status.ERR_INVALID, ["bank_process_groups", "1, 2, 4, 8 or 16"], bank, 1, d_out, 32)
    refused(Status.ERR_INVALID, ["bank_process_groups", "1, 2, 4, 8 or 16"], bank, 1, d_out, 0)
    refused(Status.ERR_INVALID, ["bank_process_groups", "input"], bank, 1, d_out, 4, in_group=4)          # no d_in
    refused(Status.ERR_INVALID, ["bank_process_groups", "null"], bank, 1, 0, 4)
    refused(Status.ERR_INVALID, ["bank_process_groups", "aligned"], bank, 1, d_out.ptr + 4, 4)
    refused(Status.ERR_INVALID, ["bank_process_groups", "layout"], bank, 1, d_out, 4, out_layout=Layout.BROADCAST)
    refused(Status.ERR_INVALID, ["bank_process_groups", "layout"], bank, 1, d_out, 4, d_in=d_out, in_layout=7)
    refused(Status.ERR_INVALID, ["bank_process_groups", "layout"], bank, 1, d_out, 4, d_in=d_out, in_layout=Layout.BROADCAST, in_group=4)
    assert_bits_equal(bank.get_all_state(), before, False, "state after refused calls")
    bank.close()

    odd = eng.bank([Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN], 72)      # 72 = 4.5 groups of 16
    refused(Status.ERR_INVALID, ["bank_process_groups", "whole"], odd, 1, d_out, 16)
    odd.process_groups(1, d_out, 8)                                       # ... and nine groups of 8
    odd.close()

    routes = ["mlgpu_bank_process", "mlgpu_mixdown_groups", "graph"]
    cascade = eng.bank([Proc.LOPASS, Proc.LOPASS], 64)
    assert cascade.fused and "cascade" in cascade.kernel_name
    eng.set_jit(False)
    try:
        unfused = eng.bank([Proc.NOISE_GEN, Proc.ONE_POLE], 64)
    finally:
        eng.set_jit(True)
    assert not unfused.fused
    for b in (cascade, unfused):
        b.process(1, d_out)
        st = b.get_all_state()
        refused(Status.ERR_UNSUPPORTED, routes, b, 1, d_out, 4)
        assert_bits_equal(b.get_all_state(), st, False, "state after an unsupported call")
        b.close()


@pytest.mark.gpu
def test_recorded_into_a_sequence(eng, oracle):
    """process_groups recorded into a sequence and launched twice gives what two direct calls give (outputs and state)."""
    ch, _, _ = reference(oracle, "bandpass", 2352, 16, False)
    C = ch.V // 16
    d_in = to_layout(eng, ch.in_rows[:, :64], Layout.QUAD, 1)
    d_gains = eng.to_device(special_gains(ch.V))
    banks, outs = [make_bank(eng, ch), make_bank(eng, ch)], [[], []]
    d_out = eng.alloc(4 * C * 64)
    for _ in range(2):
        banks[0].process_groups(1, d_out, 16, Layout.QUAD, d_in, Layout.QUAD, 16, d_gains)
        outs[0].append(d_out.download(np.float32))
    with eng.record() as seq:
        banks[1].process_groups(1, d_out, 16, Layout.QUAD, d_in, Layout.QUAD, 16, d_gains)
    assert seq.num_nodes >= 1
    for _ in range(2):
        seq.launch()
        outs[1].append(d_out.download(np.float32))
    for k in range(2):
        assert_bits_equal(outs[1][k], outs[0][k], True, f"replay {k}")
    assert np.abs(outs[0][1]).max() > 1e-6 and (outs[0][0].view(np.uint32) != outs[0][1].view(np.uint32)).any()
    assert_bits_equal(banks[1].get_all_state(), banks[0].get_all_state(), False, "state after two replays")
    for b in banks:
        b.close()


@pytest.mark.gpu
def test_cpp_wrapper_process_groups(tmp_path):
    """ml::gpu::VoiceBank::processGroups (include/mlgpu/mldsp_gpu.hpp): tests/cpp/bank_groups_test.cpp, built here against the C ABI -
    a 16-resonator bank per excitation row against operator() + mlgpu_mixdown_groups, and the shape checks."""
    from madronalib_amd import _lib
    _lib.load()
    exe = str(tmp_path / "bank_groups_test")
    lib = os.path.join(ROOT, "madronalib_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "bank_groups_test.cpp"),
           "-o", exe, "-L" + lib, "-lmlgpu", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]
