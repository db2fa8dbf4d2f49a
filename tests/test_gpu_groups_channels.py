"""The group sums per channel on the device: mlgpu_bank_process_groups_channels (chain_group_channels_kernel) and
mlgpu_bank_process_listed_groups_channels (chain_listed_group_channels_kernel) - a stereo mix per instrument, a pan gain per voice,
in the launch that advances the voices.

Expected values (groups_channels_cases): the CPU checker's voices, then the one-channel helpers of the group calls once per channel
with that channel's gains. Every comparison is of bits. Each case is also compared with the one-channel call on a twin bank prepared
identically: HIP against HIP, one step removed from the checker."""
import os
import subprocess

import numpy as np
import pytest

from groups_channels_cases import (C, CHAINS, GROUPS, LISTED_CASES, LISTED_V, SPLITS, T, VOICES, case, chain_inputs, expected_channels,
                                   expected_listed_channels, expected_peaks, listed_case, prepared)
from inputs import assert_bits_equal
from madronalib_amd.constants import Layout, Proc, Status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = np.uint32(0x7FC5A5A5)   # what the memory around an output holds before a launch


@pytest.fixture(scope="module")
def eng():
    import madronalib_amd as ml
    e = ml.Engine(0)
    yield e
    e.set_flush_denormals(False)
    e.close()


class At:
    """A place inside a device buffer (the calls read .ptr)."""

    def __init__(self, ptr):
        self.ptr = ptr


def to_layout(eng, rows, layout, vectors):
    """[R][64 vectors] numpy -> a device signal of R rows in `layout`."""
    rows = np.ascontiguousarray(rows, np.float32)
    d = eng.to_device(rows)
    if layout == Layout.VOICE_MAJOR:
        return d
    d2 = eng.alloc(rows.nbytes)
    eng.layout_convert(d, Layout.VOICE_MAJOR, d2, layout, rows.shape[0], vectors)
    return d2


def guarded(eng, words, guard_words):
    d = eng.alloc(4 * (words + guard_words))
    d.upload(np.full(words + guard_words, GUARD, np.uint32))
    return d


def rows_of(eng, d_out, offset_words, R, n, layout):
    """The signal of R rows in `layout` at d_out + offset_words -> [R][64 n] numpy."""
    if R == 0:
        return np.zeros((0, 64 * n), np.float32)
    d_vm = eng.alloc(4 * R * 64 * n)
    eng.layout_convert(At(d_out.ptr + 4 * offset_words), layout, d_vm, Layout.VOICE_MAJOR, R, n)
    return d_vm.download(np.float32, R * 64 * n).reshape(R, 64 * n)


def input_of(eng, ch, t0, n, in_layout=Layout.QUAD):
    return None if ch.in_rows is None else to_layout(eng, ch.in_rows[:, 64 * t0:64 * (t0 + n)], in_layout, n)


def make_bank(eng, ch, first_vector=False):
    """The chain's bank from clear(); first_vector: after one DSPVector of all its voices (the state groups_channels_cases.prepared has)."""
    bank = eng.bank(ch.procs, ch.V)
    bank.clear()
    bank.set_all_coeffs(ch.coeffs)
    if ch.in_const is not None:
        bank.set_input_const(ch.in_const)
    if first_vector:
        x = chain_inputs(ch)
        d_in = None if x is None else eng.to_device(np.ascontiguousarray(x[:, :64]))
        bank.process(1, eng.alloc(4 * ch.V * 64), Layout.QUAD, d_in, Layout.VOICE_MAJOR)
    return bank


def all_coeffs(bank):
    rows = [bank.get_coeff(p, i) for p in range(len(bank.procs)) for i in range(bank.num_coeffs(p))]
    return np.stack(rows) if rows else np.zeros((0, bank.V), np.float32)


# ---------------------------------------------------------------- the plain call

def run_channels(eng, bank, ch, G, splits, d_gains, out_layout=Layout.QUAD, n_channels=C):
    """process_groups_channels over launches of `splits` DSPVectors; every output - n_channels signals of V / G rows one after the
    other - has one guard row behind the last channel's region that must come back untouched. Returns [n_channels][V / G][64 T]."""
    R, outs, t0 = ch.V // G, [], 0
    for n in splits:
        d_out = guarded(eng, n_channels * R * 64 * n, 64 * n)
        bank.process_groups_channels(n, d_out, G, out_layout, input_of(eng, ch, t0, n), Layout.QUAD, ch.in_group, n_channels, d_gains)
        raw = d_out.download(np.uint32)
        assert (raw[n_channels * R * 64 * n:] == GUARD).all(), "the row behind the last channel's region was written"
        outs.append(np.stack([rows_of(eng, d_out, c * R * 64 * n, R, n, out_layout) for c in range(n_channels)]))
        t0 += n
    return np.concatenate(outs, 2)


def run_one_channel(eng, bank, ch, G, d_gains, out_layout=Layout.QUAD):
    d_out = eng.alloc(4 * (ch.V // G) * 64 * T)
    bank.process_groups(T, d_out, G, out_layout, input_of(eng, ch, 0, T), Layout.QUAD, ch.in_group, d_gains)
    return rows_of(eng, d_out, 0, ch.V // G, T, out_layout)


def check_plain(eng, oracle, name, in_group, V, G, flush=False, out_layout=Layout.QUAD):
    ch, gains, y, st = case(oracle, name, V, in_group, flush)
    want = expected_channels(oracle, y, G, gains, flush)
    what = f"{name} V={V} in_group={in_group} G={G} flush={flush} out={int(out_layout)}"
    eng.set_flush_denormals(flush)
    try:
        d_gains = eng.to_device(gains)
        bank = make_bank(eng, ch)
        one = run_channels(eng, bank, ch, G, SPLITS[0], d_gains, out_layout)
        state_one, coeffs_one = bank.get_all_state(), all_coeffs(bank)
        bank.clear()
        split = run_channels(eng, bank, ch, G, SPLITS[1], d_gains, out_layout)
        state_split = bank.get_all_state()
        bank.close()
        twins = []
        for c in range(C):    # the one-channel call with gains[c] on a twin bank prepared identically
            twin = make_bank(eng, ch)
            twins.append((run_one_channel(eng, twin, ch, G, At(d_gains.ptr + 4 * c * V), out_layout), twin.get_all_state()))
            twin.close()
    finally:
        eng.set_flush_denormals(False)
    assert np.isfinite(want).all() and np.abs(want).max() > 1e-6, what
    for c in range(C):
        assert_bits_equal(one[c], want[c], True, what + f": channel {c} of one launch against the checker")
        assert_bits_equal(one[c], twins[c][0], True, what + f": channel {c} against process_groups with gains[{c}] on a twin bank")
        assert_bits_equal(state_one, twins[c][1], False, what + f": state against the twin bank's after process_groups with gains[{c}]")
    assert_bits_equal(split, one, True, what + ": launches of 1 + 2 against one launch")
    assert_bits_equal(state_one, st, False, what + ": state against the checker's after ONE pass")
    assert_bits_equal(state_split, state_one, False, what + ": state after 1 + 2 against one launch")
    assert_bits_equal(coeffs_one, ch.coeffs, False, what + ": coefficients after the call")


@pytest.mark.gpu
@pytest.mark.parametrize("V", VOICES)
@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("name,in_group", CHAINS)
def test_two_channels_per_instrument(eng, oracle, name, in_group, G, V):
    """Groups of 2, 4, 8 (lane shifts) and 16 (the LDS strips) of SawGen -> Bandpass -> Gain on constant frequencies (the fast head,
    and the slow one where a lane sends its wavefront there) and on a streamed frequency with input groups of 1 and 4; 80 voices (a
    wavefront and a quarter: dead lanes, dead groups) and 2 352 (nine workgroups through the XCD remap, a last one of 48 voices).
    Both channels against the checker and against the one-channel call on a twin bank, the state after one pass, launches of 1 + 2,
    the guard row behind the last channel."""
    check_plain(eng, oracle, name, in_group, V, G)


@pytest.mark.gpu
@pytest.mark.parametrize("V", VOICES)
@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("name,in_group", [("saw_odd", 1), ("streamed", 4)])
def test_flushed_denormals_and_the_voice_major_output(eng, oracle, name, in_group, G, V):
    """The engine's flush-denormals mode (the gains hold a denormal: its products are flushed, in both channels' adds like every other
    add) with the output in VOICE_MAJOR, and the default mode with it too."""
    check_plain(eng, oracle, name, in_group, V, G, flush=True, out_layout=Layout.VOICE_MAJOR)
    if G in (4, 16):
        check_plain(eng, oracle, name, in_group, V, G, flush=False, out_layout=Layout.VOICE_MAJOR)


# ---------------------------------------------------------------- the listed call

def run_listed_channels(eng, bank, ch, K, J, splits, d_gains, out_layout=Layout.QUAD, n_channels=C):
    """process_listed_groups_channels with the list the bank has. Every output of n_channels * J rows has one guard row behind it, every
    d_peak[K] one guard word. Returns ([n_channels][J][64 T], the peaks [K] of each launch)."""
    outs, peaks, t0 = [], [], 0
    for n in splits:
        d_out = guarded(eng, n_channels * J * 64 * n, 64 * n)
        d_peak = guarded(eng, K, 1)
        bank.process_listed_groups_channels(n, d_out, out_layout, input_of(eng, ch, t0, n), Layout.QUAD, ch.in_group, n_channels, d_gains, d_peak)
        raw = d_out.download(np.uint32)
        assert (raw[n_channels * J * 64 * n:] == GUARD).all(), "the row behind the last channel's region was written"
        outs.append(np.stack([rows_of(eng, d_out, c * J * 64 * n, J, n, out_layout) for c in range(n_channels)]))
        pk = d_peak.download(np.uint32)
        assert pk[K] == GUARD, "the word behind d_peak[K] was written"
        peaks.append(pk[:K].copy())
        t0 += n
    return np.concatenate(outs, 2), peaks


def check_peaks(peaks, y, splits, what):
    t0 = 0
    for pk, n in zip(peaks, splits):
        assert_bits_equal(pk, expected_peaks(y[:, 64 * t0:64 * (t0 + n)]), False, f"{what}: peaks of the launch of DSPVectors {t0}..{t0 + n - 1}")
        t0 += n


@pytest.mark.gpu
@pytest.mark.parametrize("lname,G,name,in_group,flush", LISTED_CASES)
def test_listed_voices_in_two_channels_per_instrument(eng, oracle, lname, G, name, in_group, flush):
    """Rows [2][J] against the checker, the peaks [K] - taken before any gain - with their guard word, the guard row behind the last
    channel, every state and coefficient word of the unlisted voices unchanged, the listed voices' state after ONE pass, launches of
    1 + 2. With every voice listed: the bits of process_groups_channels of a twin bank. With none: MLGPU_OK and nothing written."""
    ch, gains, L, st0, y, st = listed_case(oracle, lname, name, in_group, flush)
    V, K, rest = LISTED_V, L.size, np.setdiff1d(np.arange(LISTED_V), L)
    want, M = expected_listed_channels(oracle, y, L, G, gains, flush)
    J = M.size
    what = f"{name} list={lname} K={K} G={G} in_group={in_group} flush={flush}"
    eng.set_flush_denormals(flush)
    try:
        d_gains = eng.to_device(gains)
        bank = make_bank(eng, ch, first_vector=True)
        bank.reserve_voice_list_groups(max(K, 1), G)
        bank.set_voice_list(L)
        got_M = bank.listed_groups
        before = (bank.get_all_state(), all_coeffs(bank), bank.get_input_const())
        one, peaks_one = run_listed_channels(eng, bank, ch, K, J, SPLITS[0], d_gains)
        after = (bank.get_all_state(), all_coeffs(bank), bank.get_input_const())
        bank.set_all_state(before[0])
        split, peaks_split = run_listed_channels(eng, bank, ch, K, J, SPLITS[1], d_gains, Layout.VOICE_MAJOR)
        state_split = bank.get_all_state()
        bank.close()
        plain = None
        if lname == "all":
            twin = make_bank(eng, ch, first_vector=True)
            plain = (run_channels(eng, twin, ch, G, SPLITS[0], d_gains), twin.get_all_state())
            twin.close()
    finally:
        eng.set_flush_denormals(False)
    assert (got_M == M).all() and got_M.shape == M.shape, what + ": listed_groups"
    assert_bits_equal(before[0], st0, False, what + ": state before the call against the checker")
    if K:
        assert np.isfinite(want).all() and np.abs(want).max() > 1e-6, what
    else:
        assert one.shape == (C, 0, 64 * T)
    for c in range(C):
        assert_bits_equal(one[c], want[c], True, what + f": channel {c} of one launch against the checker")
    assert_bits_equal(split, one, True, what + ": launches of 1 + 2 (VOICE_MAJOR) against one launch (QUAD)")
    check_peaks(peaks_one, y, SPLITS[0], what)
    check_peaks(peaks_split, y, SPLITS[1], what + " (1 + 2)")
    assert_bits_equal(after[0][:, L], st[:, L], False, what + ": state of the listed voices against the checker's after ONE pass")
    assert_bits_equal(after[0][:, rest], before[0][:, rest], False, what + ": state of the unlisted voices against the download before the call")
    assert_bits_equal(after[1], before[1], False, what + ": coefficients against the download before the call")
    assert_bits_equal(after[2], before[2], False, what + ": input constants against the download before the call")
    assert_bits_equal(state_split, after[0], False, what + ": state after 1 + 2 against one launch")
    if plain is not None:
        assert_bits_equal(one, plain[0], True, what + ": every voice listed against process_groups_channels of a twin bank")
        assert_bits_equal(after[0], plain[1], False, what + ": state against process_groups_channels of a twin bank")


# ---------------------------------------------------------------- one channel, errors, recording, the C++ wrapper

@pytest.mark.gpu
def test_one_channel_is_the_one_channel_call(eng, oracle):
    """n_channels == 1 gives the bits (output and state) of process_groups / process_listed_groups, with gains and with NULL gains."""
    ch, gains, _, _ = case(oracle, "saw_odd", 80)
    for g in (gains[1], None):
        d_g = None if g is None else eng.to_device(np.ascontiguousarray(g))
        a, b = make_bank(eng, ch), make_bank(eng, ch)
        got = run_channels(eng, a, ch, 16, SPLITS[0], d_g, n_channels=1)[0]
        want = run_one_channel(eng, b, ch, 16, d_g)
        assert np.abs(want).max() > 1e-6
        assert_bits_equal(got, want, True, f"plain, gains={g is not None}")
        assert_bits_equal(a.get_all_state(), b.get_all_state(), False, "plain: state")
        a.close(), b.close()
    ch, gains, L, _, _, _ = listed_case(oracle, "straddle", "saw")
    for g in (gains[1], None):
        d_g = None if g is None else eng.to_device(np.ascontiguousarray(g))
        outs = []
        for channels_call in (True, False):
            bank = make_bank(eng, ch, first_vector=True)
            bank.reserve_voice_list_groups(L.size, 16)
            bank.set_voice_list(L)
            J = bank.listed_groups.size
            d_out, d_peak = eng.alloc(4 * J * 64 * T), eng.alloc(4 * L.size)
            if channels_call:
                bank.process_listed_groups_channels(T, d_out, Layout.QUAD, n_channels=1, d_gains=d_g, d_peak=d_peak)
            else:
                bank.process_listed_groups(T, d_out, Layout.QUAD, d_gains=d_g, d_peak=d_peak)
            outs.append((d_out.download(np.float32), d_peak.download(np.uint32), bank.get_all_state()))
            bank.close()
        assert np.abs(outs[1][0]).max() > 1e-6
        assert_bits_equal(outs[0][0], outs[1][0], True, f"listed, gains={g is not None}")
        assert_bits_equal(outs[0][1], outs[1][1], False, "listed: peaks")
        assert_bits_equal(outs[0][2], outs[1][2], False, "listed: state")


def refused(status, words, fn, *args, **kw):
    import madronalib_amd as ml
    with pytest.raises(ml.MlgpuError) as ei:
        fn(*args, **kw)
    assert ei.value.status == status, str(ei.value)
    assert all(w in str(ei.value) for w in words), str(ei.value)


def other_banks(eng):
    """Banks whose chains have no group form per channel: a single processor (it has the one-channel group form), an SVF cascade, a
    processor-by-processor bank."""
    single = eng.bank([Proc.BANDPASS], 64)
    cascade = eng.bank([Proc.LOPASS, Proc.LOPASS], 64)
    assert cascade.fused and "cascade" in cascade.kernel_name
    eng.set_jit(False)
    try:
        unfused = eng.bank([Proc.NOISE_GEN, Proc.ONE_POLE], 64)
    finally:
        eng.set_jit(True)
    assert not unfused.fused
    return single, cascade, unfused


ROUTE = ["graph", "two group-summed outputs"]


@pytest.mark.gpu
def test_refusals_of_the_plain_call_in_their_order(eng, oracle):
    """MLGPU_ERR_UNSUPPORTED for the channel count (and for a group of 1, which has nothing to sum) before anything else; then the
    one-channel call's checks in its order, null gains after the groups and before the signals; MLGPU_ERR_UNSUPPORTED for a bank without
    the form last. After each refused call the output holds its guard words and the state its bits, and a valid call follows."""
    ch, gains, y, _ = case(oracle, "saw", 80)
    V, G, call = 80, 16, "bank_process_groups_channels"
    bank = make_bank(eng, ch)
    d_gains = eng.to_device(gains)
    d_out = guarded(eng, C * (V // 2) * 64 * T, 0)
    before = bank.get_all_state()
    f = bank.process_groups_channels
    for count in (0, 3, -1):     # 1. the channel count, whatever else is wrong
        refused(Status.ERR_UNSUPPORTED, [call, "1 or 2 channels"], f, T, d_out, 3, n_channels=count, d_gains=None)
    refused(Status.ERR_UNSUPPORTED, [call, "nothing to sum"], f, T, 0, 1, n_channels=2, d_gains=None)
    # 2. the one-channel call's checks, in its order
    refused(Status.ERR_INVALID, [call, "1, 2, 4, 8 or 16"], f, T, 0, 3, n_channels=2, d_gains=None)
    refused(Status.ERR_INVALID, [call, "1, 2, 4, 8 or 16"], f, T, d_out, G, d_in=d_out, in_group=3, n_channels=2, d_gains=d_gains)
    refused(Status.ERR_INVALID, [call, "streamed input"], f, T, 0, G, in_group=4, n_channels=2, d_gains=None)
    refused(Status.ERR_INVALID, [call, "null gains"], f, T, 0, G, n_channels=2, d_gains=None)         # (before the null output)
    refused(Status.ERR_INVALID, [call, "null output"], f, T, 0, G, n_channels=2, d_gains=d_gains)
    refused(Status.ERR_INVALID, [call, "layout"], f, T, d_out, G, Layout.BROADCAST, n_channels=2, d_gains=d_gains)
    refused(Status.ERR_INVALID, [call, "layout"], f, T, d_out, G, d_in=d_out, in_layout=7, n_channels=2, d_gains=d_gains)
    refused(Status.ERR_INVALID, [call, "aligned"], f, T, At(d_out.ptr + 4), G, n_channels=2, d_gains=d_gains)
    refused(Status.ERR_INVALID, [call, "misaligned gains"], f, T, d_out, G, n_channels=2, d_gains=At(d_gains.ptr + 2))
    assert (d_out.download(np.uint32) == GUARD).all(), "a refused call wrote the output"
    assert_bits_equal(bank.get_all_state(), before, False, "state after refused calls")
    odd = eng.bank([Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN], 72)      # 72 = 4.5 groups of 16
    refused(Status.ERR_INVALID, [call, "whole number"], odd.process_groups_channels, 1, d_out, 16, n_channels=2, d_gains=d_gains)
    odd.close()
    # 3. a bank without the form: last, after its arguments have been looked at
    for b in other_banks(eng):
        b.process(1, eng.alloc(4 * 64 * 64), Layout.QUAD, d_out if b.procs[0] in (Proc.BANDPASS, Proc.LOPASS) else None)
        st = b.get_all_state()
        refused(Status.ERR_INVALID, [call, "null output"], b.process_groups_channels, 1, 0, 4, n_channels=2, d_gains=d_gains)
        refused(Status.ERR_UNSUPPORTED, [call] + ROUTE, b.process_groups_channels, 1, d_out, 4, n_channels=2, d_gains=d_gains)
        assert_bits_equal(b.get_all_state(), st, False, "state after an unsupported call")
        b.close()
    assert (d_out.download(np.uint32) == GUARD).all(), "a refused call wrote the output"
    # ... and the valid call that follows
    got = run_channels(eng, bank, ch, G, SPLITS[0], d_gains)
    assert_bits_equal(got, expected_channels(oracle, y, G, gains), True, "the valid call after the refused ones")
    bank.close()


@pytest.mark.gpu
def test_refusals_of_the_listed_call_in_their_order(eng, oracle):
    ch, gains, L, st0, y, _ = listed_case(oracle, "straddle", "saw")
    G, call = 16, "bank_process_listed_groups_channels"
    want, M = expected_listed_channels(oracle, y, L, G, gains)
    bank = make_bank(eng, ch, first_vector=True)
    d_gains = eng.to_device(gains)
    d_out = guarded(eng, C * M.size * 64 * T, 0)
    bank.reserve_voice_list(L.size)
    bank.set_voice_list(L)
    f = bank.process_listed_groups_channels
    refused(Status.ERR_UNSUPPORTED, [call, "1 or 2 channels"], f, T, 0, n_channels=3, d_gains=None)            # 1. the count, before the missing reserve
    refused(Status.ERR_INVALID, [call, "reserve_voice_list_groups"], f, T, 0, n_channels=2, d_gains=None)      # 2. the one-channel call's order
    bank.reserve_voice_list_groups(L.size, G)
    with eng.record():
        refused(Status.ERR_INVALID, [call, "recording", "contents"], f, T, d_out, n_channels=2, d_gains=d_gains)
    refused(Status.ERR_INVALID, [call, "groups of"], f, T, 0, in_group=3, n_channels=2, d_gains=None)
    refused(Status.ERR_INVALID, [call, "streamed input"], f, T, 0, in_group=4, n_channels=2, d_gains=None)
    refused(Status.ERR_INVALID, [call, "null gains"], f, T, 0, n_channels=2, d_gains=None)
    refused(Status.ERR_INVALID, [call, "null output"], f, T, 0, n_channels=2, d_gains=d_gains)
    refused(Status.ERR_INVALID, [call, "layout"], f, T, d_out, Layout.BROADCAST, n_channels=2, d_gains=d_gains)
    refused(Status.ERR_INVALID, [call, "aligned"], f, T, At(d_out.ptr + 4), n_channels=2, d_gains=d_gains)
    refused(Status.ERR_INVALID, [call, "peaks or gains"], f, T, d_out, n_channels=2, d_gains=At(d_gains.ptr + 2))
    refused(Status.ERR_INVALID, [call, "peaks or gains"], f, T, d_out, n_channels=2, d_gains=d_gains, d_peak=At(d_out.ptr + 2))
    assert (d_out.download(np.uint32) == GUARD).all(), "a refused call wrote the output"
    assert_bits_equal(bank.get_all_state(), st0, False, "state after refused calls")
    for b in other_banks(eng):     # 3. a bank without the form
        b.process(1, eng.alloc(4 * 64 * 64), Layout.QUAD, d_out if b.procs[0] in (Proc.BANDPASS, Proc.LOPASS) else None)
        b.reserve_voice_list_groups(8, 16)
        b.set_voice_list([1, 5, 63])
        st = b.get_all_state()
        refused(Status.ERR_UNSUPPORTED, [call] + ROUTE, b.process_listed_groups_channels, 1, d_out, n_channels=2, d_gains=d_gains)
        assert_bits_equal(b.get_all_state(), st, False, "state after an unsupported call")
        b.close()
    assert (d_out.download(np.uint32) == GUARD).all(), "a refused call wrote the output"
    got, _ = run_listed_channels(eng, bank, ch, L.size, M.size, SPLITS[0], d_gains)
    assert_bits_equal(got, want, True, "the valid call after the refused ones")
    bank.close()


@pytest.mark.gpu
def test_recorded_into_a_sequence(eng, oracle):
    """process_groups_channels recorded into a sequence and launched twice gives what two direct calls give (outputs and state)."""
    ch, gains, _, _ = case(oracle, "streamed", 2352, 4)
    R = ch.V // 16
    d_in = to_layout(eng, ch.in_rows[:, :64], Layout.QUAD, 1)
    d_gains = eng.to_device(gains)
    banks, outs = [make_bank(eng, ch), make_bank(eng, ch)], [[], []]
    d_out = eng.alloc(4 * C * R * 64)
    for _ in range(2):
        banks[0].process_groups_channels(1, d_out, 16, Layout.QUAD, d_in, Layout.QUAD, 4, C, d_gains)
        outs[0].append(d_out.download(np.float32))
    with eng.record() as seq:
        banks[1].process_groups_channels(1, d_out, 16, Layout.QUAD, d_in, Layout.QUAD, 4, C, d_gains)
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
def test_cpp_wrapper_process_groups_channels(tmp_path):
    """ml::gpu::VoiceBank::processGroupsChannels (include/mlgpu/mldsp_gpu.hpp): tests/cpp/groups_channels_test.cpp, built here against
    the C ABI - each channel against processGroups of an identical bank with that channel's gains, one channel, and the shape checks."""
    from madronalib_amd import _lib
    _lib.load()
    exe = str(tmp_path / "groups_channels_test")
    lib = os.path.join(ROOT, "madronalib_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "groups_channels_test.cpp"),
           "-o", exe, "-L" + lib, "-lmlgpu", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]
