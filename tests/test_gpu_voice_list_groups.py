"""The listed group sum on the device: mlgpu_bank_reserve_voice_list_groups, mlgpu_bank_process_listed_groups (chain_listed_group_kernel) -
one row per listed instrument, the in-order sum of that instrument's listed voices, and nobody else is touched.

Expected values (voice_list_groups_cases): the CPU checker's chain_process on the K listed voices (voice_list_cases.expected_listed),
each row times its voice's gain, accumulated per instrument from +0.0 with the checker's float32 add; the peaks in numpy on the voices'
own samples. Every bank first runs one DSPVector on ALL its voices (and so does the checker), so that the state an unlisted voice must
keep is not the cleared one. Every comparison is of bits."""
import numpy as np
import pytest

from inputs import assert_bits_equal
from madronalib_amd.constants import Layout, Proc, Status
from voice_list_groups_cases import (Chain, T, V, expected_listed, expected_listed_groups, expected_peaks, group_lists, listed_instruments, special_gains)
from voice_list_cases import chain_inputs, expected_listed_mixdown

GUARD = np.uint32(0x7FC5A5A5)   # what the memory around an output holds before a launch
LISTS = group_lists()
_prepared, _expected = {}, {}


@pytest.fixture(scope="module")
def eng():
    import madronalib_amd as ml
    e = ml.Engine(0)
    e.mixdown_reserve(V, T)
    yield e
    e.set_flush_denormals(False)
    e.close()


def prepared(oracle, name, in_group=1, flush=False):
    """(chain, the checker's state after one DSPVector of all V voices from clear()), once per chain, input group and mode."""
    key = (name, in_group, flush)
    if key not in _prepared:
        ch = Chain(name, oracle, V, in_group)
        st0 = oracle.chain_clear(ch.procs, V)
        x = chain_inputs(ch)
        with oracle.flush_denormals(flush):
            oracle.chain_process(ch.procs, 1, ch.coeffs, st0, None if x is None else np.ascontiguousarray(x[:, :64]), ch.in_const, n_threads=4, want_out=False)
        st0.setflags(write=False)
        _prepared[key] = (ch, st0)
    return _prepared[key]


def reference(oracle, name, lname, in_group=1, flush=False):
    """(chain, state before, the listed voices' signals [K][64 T], the full state after) for one launch of T DSPVectors."""
    key = (name, lname, in_group, flush)
    if key not in _expected:
        ch, st0 = prepared(oracle, name, in_group, flush)
        st = st0.copy()
        y = expected_listed(oracle, ch, LISTS[lname], st, 0, T, flush)
        y.setflags(write=False), st.setflags(write=False)
        _expected[key] = (ch, st0, y, st)
    return _expected[key]


def to_layout(eng, rows, layout, vectors):
    """[R][64 vectors] numpy -> a device signal of R rows in `layout`."""
    rows = np.ascontiguousarray(rows, np.float32)
    d = eng.to_device(rows)
    if layout == Layout.VOICE_MAJOR:
        return d
    d2 = eng.alloc(rows.nbytes)
    eng.layout_convert(d, Layout.VOICE_MAJOR, d2, layout, rows.shape[0], vectors)
    return d2


def make_bank(eng, ch):
    """The chain's bank after one DSPVector of all its voices (the state `prepared` has)."""
    bank = eng.bank(ch.procs, ch.V)
    bank.clear()
    bank.set_all_coeffs(ch.coeffs)
    if ch.in_const is not None:
        bank.set_input_const(ch.in_const)
    x = chain_inputs(ch)
    d_in = None if x is None else eng.to_device(np.ascontiguousarray(x[:, :64]))
    bank.process(1, eng.alloc(4 * ch.V * 64), Layout.QUAD, d_in, Layout.VOICE_MAJOR)
    return bank


def all_coeffs(bank):
    rows = [bank.get_coeff(p, i) for p in range(len(bank.procs)) for i in range(bank.num_coeffs(p))]
    return np.stack(rows) if rows else np.zeros((0, bank.V), np.float32)


def guarded(eng, words, guard_words):
    d = eng.alloc(4 * (words + guard_words))
    d.upload(np.full(words + guard_words, GUARD, np.uint32))
    return d


def run_groups(eng, bank, ch, K, J, splits, out_layout=Layout.QUAD, in_layout=Layout.QUAD, d_gains=None):
    """process_listed_groups over launches of `splits` DSPVectors with the list the bank has. Every output of J rows has one guard row
    behind it, every d_peak[K] one guard word, that must come back untouched. Returns ([J][64 T], the peaks [K] of each launch)."""
    outs, peaks, t0 = [], [], 0
    for n in splits:
        d_in = None if ch.in_rows is None else to_layout(eng, ch.in_rows[:, 64 * t0:64 * (t0 + n)], in_layout, n)   # V / in_group rows
        d_out = guarded(eng, J * 64 * n, 64 * n)
        d_peak = guarded(eng, K, 1)
        bank.process_listed_groups(n, d_out, out_layout, d_in, in_layout, ch.in_group, d_gains, d_peak)
        raw = d_out.download(np.uint32)
        assert (raw[J * 64 * n:] == GUARD).all(), "the row behind the output was written"
        if J == 0:
            outs.append(np.zeros((0, 64 * n), np.float32))
        else:
            d_vm = eng.alloc(4 * J * 64 * n)
            eng.layout_convert(d_out, out_layout, d_vm, Layout.VOICE_MAJOR, J, n)
            outs.append(d_vm.download(np.float32, J * 64 * n).reshape(J, 64 * n))
        pk = d_peak.download(np.uint32)
        assert pk[K] == GUARD, "the word behind d_peak[K] was written"
        peaks.append(pk[:K].copy())
        t0 += n
    return np.concatenate(outs, 1), peaks


def check_peaks(peaks, y, splits, what):
    t0 = 0
    for pk, n in zip(peaks, splits):
        assert_bits_equal(pk, expected_peaks(y[:, 64 * t0:64 * (t0 + n)]), False, f"{what}: peaks of the launch of DSPVectors {t0}..{t0 + n - 1}")
        t0 += n


def check_groups(eng, oracle, name, lname, G, in_group=1, with_gains=False, flush=False, out_layout=Layout.QUAD, in_layout=Layout.QUAD,
                 list_before_reserve=False):
    ch, st0, y, st = reference(oracle, name, lname, in_group, flush)
    L = LISTS[lname]
    K, rest = L.size, np.setdiff1d(np.arange(V), L)
    gains = special_gains(V) if with_gains else None
    want, M = expected_listed_groups(oracle, y, L, G, gains, flush)
    J = M.size
    what = f"{name} list={lname} K={K} G={G} in_group={in_group} gains={with_gains} flush={flush} out={int(out_layout)} in={int(in_layout)}"
    eng.set_flush_denormals(flush)
    try:
        d_gains = None if gains is None else eng.to_device(gains)
        bank = make_bank(eng, ch)
        if list_before_reserve:    # the list in force gets its plan in the reserve call
            bank.set_voice_list(L)
            bank.reserve_voice_list_groups(max(K, 1), G)
        else:
            bank.reserve_voice_list_groups(max(K, 1), G)
            bank.set_voice_list(L)
        assert bank.voice_list_size == K
        got_M = bank.listed_groups
        before = (bank.get_all_state(), all_coeffs(bank), bank.get_input_const())
        one, peaks_one = run_groups(eng, bank, ch, K, J, [T], out_layout, in_layout, d_gains)
        after = (bank.get_all_state(), all_coeffs(bank), bank.get_input_const())
        bank.set_all_state(before[0])
        split, peaks_split = run_groups(eng, bank, ch, K, J, [1, T - 1], out_layout, in_layout, d_gains)
        state_split = bank.get_all_state()
        bank.close()
    finally:
        eng.set_flush_denormals(False)
    assert got_M.dtype == np.uint32 and got_M.shape == M.shape and (got_M == M).all(), what + ": listed_groups"
    assert_bits_equal(before[0], st0, False, what + ": state before the call against the oracle")
    if K:
        assert np.isfinite(want).all() and np.abs(want).max() > 1e-6, what
    assert_bits_equal(one, want, True, what + ": one launch against the oracle's voices summed by instrument")
    assert_bits_equal(split, one, True, what + ": launches of 1 + 2 against one launch")
    check_peaks(peaks_one, y, [T], what)          # (the voice's own sample: before the gain)
    check_peaks(peaks_split, y, [1, T - 1], what + " (1 + 2)")
    assert_bits_equal(after[0][:, L], st[:, L], False, what + ": state of the listed voices against the oracle")
    assert_bits_equal(after[0][:, rest], before[0][:, rest], False, what + ": state of the unlisted voices against the download before the call")
    assert_bits_equal(after[1], before[1], False, what + ": coefficients against the download before the call")
    assert_bits_equal(after[2], before[2], False, what + ": input constants against the download before the call")
    assert_bits_equal(state_split, after[0], False, what + ": state after 1 + 2 against one launch")


@pytest.mark.gpu
@pytest.mark.parametrize("lname", ["straddle", "fit", "k2100", "last"])
@pytest.mark.parametrize("name", ["saw", "saw_odd", "bandpass", "impulse"])
def test_listed_voices_summed_by_instrument(eng, oracle, name, lname):
    """G = 16 over V = 2352. SawGen -> Bandpass -> Gain with the trip head (saw) and with voices 5 and V - 3 sending their wavefronts
    to the slow head when listed (saw_odd), Bandpass on a streamed input of V rows, ImpulseGen (its LDS table and workgroup barrier
    ahead of any lane's exit, beside the strip). Lists: straddle (a segment that does not fit: two pad lanes in the first wavefront),
    fit (a segment ends at lane 63, a full one follows), k2100 (248 pads, ten workgroups, eight through the XCD remap) and the last
    voice alone. Rows with their guard row, listed_groups, the peaks by list position and their guard word, the listed voices' state
    against the oracle, every state, coefficient and input-constant word against a download taken before the call, and launches of
    1 + 2 DSPVectors against one of 3."""
    check_groups(eng, oracle, name, lname, 16)


@pytest.mark.gpu
@pytest.mark.parametrize("lname", ["k2100", "straddle"])
@pytest.mark.parametrize("G", [2, 4, 8])
def test_every_group_size(eng, oracle, G, lname):
    """The group size is data of the plan. Here the list is set first: the reserve call makes the plan of the list in force."""
    check_groups(eng, oracle, "saw", lname, G, list_before_reserve=True)


@pytest.mark.gpu
def test_a_wavefront_on_the_fast_head_beside_one_in_trips(eng, oracle):
    """The head mode no other case of this form reaches: a constant frequency above 1/16 in a lane sends its wavefront to the fast
    per-sample head, neither trips nor the range test. V = 80, G = 16, T = 3: the first wavefront (64 lanes, four instruments, voice 3
    unlisted) makes trips, the ragged second one (16 lanes, voice 70 unlisted) has three lanes above 1/16. Rows, peaks and the
    listed voices' state against the oracle as in check_groups; the unlisted voices' state against a download before the call."""
    Vs, G = 80, 16
    ch = Chain("saw", oracle, Vs)
    freq = ch.in_const.copy()
    assert ((freq > 0) & (freq <= np.float32(1.0 / 16.0))).all()          # (as the chain comes: trips everywhere)
    freq[[66, 71, 79]] = np.array([0.07, 0.11, 0.2], np.float32)
    ch.in_const = freq
    L = np.setdiff1d(np.arange(Vs), [3, 70]).astype(np.uint32)
    K, rest = L.size, np.array([3, 70])
    st0 = oracle.chain_clear(ch.procs, Vs)
    oracle.chain_process(ch.procs, 1, ch.coeffs, st0, None, freq, n_threads=4, want_out=False)    # (make_bank's DSPVector of all voices)
    st = st0.copy()
    y = expected_listed(oracle, ch, L, st, 0, T)
    want, M = expected_listed_groups(oracle, y, L, G)
    bank = make_bank(eng, ch)
    bank.reserve_voice_list_groups(K, G)
    bank.set_voice_list(L)
    before = bank.get_all_state()
    got, peaks = run_groups(eng, bank, ch, K, M.size, [T])
    after = bank.get_all_state()
    bank.close()
    assert M.size == Vs // G and np.isfinite(want).all() and np.abs(want).max() > 1e-6
    assert_bits_equal(before, st0, False, "state before the call against the oracle")
    assert_bits_equal(got, want, True, "one launch against the oracle's voices summed by instrument")
    check_peaks(peaks, y, [T], "fast head")
    assert_bits_equal(after[:, L], st[:, L], False, "state of the listed voices against the oracle")
    assert_bits_equal(after[:, rest], before[:, rest], False, "state of the unlisted voices against the download before the call")


@pytest.mark.gpu
def test_an_input_group_is_read_at_the_voice(eng, oracle):
    """in_group 4: the streamed input has V / 4 rows and voice v reads row v // 4, listed or not."""
    check_groups(eng, oracle, "bandpass", "k2100", 16, in_group=4)


@pytest.mark.gpu
@pytest.mark.parametrize("flush", [pytest.param(False, id="ieee"), pytest.param(True, id="flush")])
def test_gains_in_both_float_modes(eng, oracle, flush):
    """special_gains (a -0.0, a 0.0 and a denormal among them), indexed by voice, one multiply before the adds; the peaks stay those
    of the voice's own sample."""
    check_groups(eng, oracle, "saw_odd", "k2100", 16, with_gains=True, flush=flush)
    if not flush:
        check_groups(eng, oracle, "saw", "all", 16, with_gains=True)   # (voices 1, 2, 5 and their like at the end: all listed)


@pytest.mark.gpu
def test_no_gains_is_no_multiply(eng, oracle):
    """d_gains = NULL: the rows are the helper's without gains - here in flush mode, the other cases without gains in the default one."""
    check_groups(eng, oracle, "saw", "k2100", 16, flush=True)


@pytest.mark.gpu
@pytest.mark.parametrize("out_layout,in_layout", [(Layout.VOICE_MAJOR, Layout.VOICE_MAJOR), (Layout.QUAD, Layout.VOICE_MAJOR), (Layout.VOICE_MAJOR, Layout.QUAD)])
def test_layouts(eng, oracle, out_layout, in_layout):
    check_groups(eng, oracle, "bandpass", "k2100", 16, out_layout=out_layout, in_layout=in_layout)
    check_groups(eng, oracle, "saw", "straddle", 16, out_layout=out_layout)


@pytest.mark.gpu
def test_a_broadcast_row_is_read_as_process_reads_it(eng, oracle):
    """MLGPU_LAYOUT_BROADCAST with in_group 1: one row for every voice - the same bits as that row given per voice."""
    ch, _ = prepared(oracle, "bandpass")
    L = LISTS["k2100"]
    J = listed_instruments(L, 16)[0].size
    row = np.ascontiguousarray(chain_inputs(ch)[3])
    outs = []
    for d_in, layout in ((eng.to_device(row), Layout.BROADCAST), (eng.to_device(np.ascontiguousarray(np.repeat(row[None, :], V, axis=0))), Layout.VOICE_MAJOR)):
        bank = make_bank(eng, ch)
        bank.reserve_voice_list_groups(L.size, 16)
        bank.set_voice_list(L)
        d_out = eng.alloc(4 * J * 64 * T)
        bank.process_listed_groups(T, d_out, Layout.VOICE_MAJOR, d_in, layout)
        outs.append(d_out.download(np.float32))
        bank.close()
    assert_bits_equal(outs[0], outs[1], True, "a broadcast input against the same row per voice")
    assert np.abs(outs[0]).max() > 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("G", [2, 4, 8, 16])
def test_every_voice_listed_is_process_groups(eng, oracle, G):
    """The list of all voices: no pads, and the bits (rows and state) of mlgpu_bank_process_groups of an identical second bank."""
    ch, _ = prepared(oracle, "saw_odd")
    L = LISTS["all"]
    gains = special_gains(V)
    for g in (None, gains):
        d_gains = None if g is None else eng.to_device(g)
        a, b = make_bank(eng, ch), make_bank(eng, ch)
        a.reserve_voice_list_groups(V, G)
        a.set_voice_list(L)
        assert (a.listed_groups == np.arange(V // G)).all()
        d_a, d_b = eng.alloc(4 * (V // G) * 64 * T), eng.alloc(4 * (V // G) * 64 * T)
        a.process_listed_groups(T, d_a, Layout.QUAD, d_gains=d_gains)
        b.process_groups(T, d_b, G, Layout.QUAD, d_gains=d_gains)
        out_a, out_b = d_a.download(np.float32), d_b.download(np.float32)
        assert np.abs(out_b).max() > 1e-6
        assert_bits_equal(out_a, out_b, True, f"G={G} gains={g is not None}: against process_groups of a second bank")
        assert_bits_equal(a.get_all_state(), b.get_all_state(), False, f"G={G}: state against process_groups of a second bank")
        a.close(), b.close()


@pytest.mark.gpu
def test_the_other_listed_calls_keep_their_bits_after_the_groups_reserve(eng, oracle):
    """After reserve_voice_list_groups, process_listed and process_listed_mixdown of the same list still give the helpers' bits."""
    ch, st0, y, st = reference(oracle, "saw", "k2100")
    L = LISTS["k2100"]
    gains = special_gains(V)
    bank = make_bank(eng, ch)
    bank.reserve_voice_list_groups(L.size, 16)
    bank.set_voice_list(L)
    d_out = eng.alloc(4 * L.size * 64 * T)
    bank.process_listed(T, d_out, Layout.VOICE_MAJOR)
    assert_bits_equal(d_out.download(np.float32).reshape(L.size, 64 * T), y, True, "process_listed after the groups reserve")
    assert_bits_equal(bank.get_all_state(), st, False, "state")
    bank.set_all_state(st0)
    d_mix = eng.alloc(4 * 64 * T)
    bank.process_listed_mixdown(T, d_mix, d_gains=eng.to_device(gains))
    assert_bits_equal(d_mix.download(np.float32, 64 * T), expected_listed_mixdown(oracle, y, L, gains), True, "process_listed_mixdown after the groups reserve")
    assert_bits_equal(bank.get_all_state(), st, False, "state")
    # ... and out_group 0 turns the plan off again
    bank.reserve_voice_list_groups(L.size, 0)
    assert bank.listed_groups.size == 0
    refused(Status.ERR_INVALID, ["bank_process_listed_groups", "reserve_voice_list_groups"], bank.process_listed_groups, T, d_out)
    bank.close()


@pytest.mark.gpu
def test_a_list_change_between_two_calls_is_ordered_on_the_stream(eng, oracle):
    """set_voice_list(straddle), process, set_voice_list(fit), process - one DSPVector each, nothing waited for in between. The two
    lists have different lengths, lane counts (76, 81) and instrument counts (71, 63): the second call's rows and listed_groups belong
    to the new list, and every voice has advanced by exactly the blocks it was listed in."""
    ch, st0 = prepared(oracle, "saw")
    A, B = LISTS["straddle"], LISTS["fit"]
    (MA, _), (MB, _) = listed_instruments(A, 16), listed_instruments(B, 16)
    bank = make_bank(eng, ch)
    bank.reserve_voice_list_groups(max(A.size, B.size), 16)
    d_a, d_b = guarded(eng, MA.size * 64, 64), guarded(eng, MB.size * 64, 64)
    p_a, p_b = eng.alloc(4 * A.size), eng.alloc(4 * B.size)
    bank.set_voice_list(A)
    groups_a = bank.listed_groups
    bank.process_listed_groups(1, d_a, Layout.VOICE_MAJOR, d_peak=p_a)
    bank.set_voice_list(B)
    groups_b = bank.listed_groups
    bank.process_listed_groups(1, d_b, Layout.VOICE_MAJOR, d_peak=p_b)
    got_a, got_b = d_a.download(np.uint32), d_b.download(np.uint32)
    peaks_a, peaks_b = p_a.download(np.uint32), p_b.download(np.uint32)
    state = bank.get_all_state()
    bank.close()
    assert (groups_a == MA).all() and groups_b.shape == MB.shape and (groups_b == MB).all()
    st = st0.copy()
    ya = expected_listed(oracle, ch, A, st, 0, 1)
    yb = expected_listed(oracle, ch, B, st, 0, 1)
    assert (got_a[MA.size * 64:] == GUARD).all() and (got_b[MB.size * 64:] == GUARD).all()
    assert_bits_equal(got_a[:MA.size * 64].view(np.float32).reshape(MA.size, 64), expected_listed_groups(oracle, ya, A, 16)[0], True, "the block of straddle")
    assert_bits_equal(got_b[:MB.size * 64].view(np.float32).reshape(MB.size, 64), expected_listed_groups(oracle, yb, B, 16)[0], True, "the block of fit")
    assert_bits_equal(peaks_a, expected_peaks(ya), False, "the peaks of straddle")
    assert_bits_equal(peaks_b, expected_peaks(yb), False, "the peaks of fit")
    assert_bits_equal(state, st, False, "final state: every voice advanced by exactly the blocks it was listed in")


def refused(status, words, fn, *args, **kw):
    import madronalib_amd as ml
    with pytest.raises(ml.MlgpuError) as ei:
        fn(*args, **kw)
    assert ei.value.status == status, str(ei.value)
    assert all(w in str(ei.value) for w in words), str(ei.value)


@pytest.mark.gpu
def test_refusals_leave_the_output_and_the_state_untouched(eng, oracle):
    """MLGPU_ERR_INVALID: no groups reserve, an in_group that is no group size, an input group without d_in or with a broadcast input,
    null / misaligned / badly laid out arguments, a call while recording a sequence. MLGPU_ERR_UNSUPPORTED: a processor-by-processor
    bank and an SVF cascade bank. MLGPU_OK with nothing written: the empty list. After each, the output buffer holds its guard words
    and the state its bits."""
    ch, st0 = prepared(oracle, "saw")
    L = LISTS["straddle"]
    words = 71 * 64 * T
    d_out = guarded(eng, words, 0)

    def untouched(bank, state, what):
        assert (d_out.download(np.uint32) == GUARD).all(), what + ": the output buffer was written"
        assert_bits_equal(bank.get_all_state(), state, False, what + ": state")

    bank = make_bank(eng, ch)
    bank.reserve_voice_list(L.size)
    bank.set_voice_list(L)
    refused(Status.ERR_INVALID, ["bank_process_listed_groups", "reserve_voice_list_groups"], bank.process_listed_groups, T, d_out)
    untouched(bank, st0, "no groups reserve")
    refused(Status.ERR_INVALID, ["bank_reserve_voice_list_groups"], bank.reserve_voice_list_groups, L.size, 3)
    bank.reserve_voice_list_groups(L.size, 16)
    assert bank.listed_groups.size == 71
    refused(Status.ERR_INVALID, ["bank_process_listed_groups", "groups of"], bank.process_listed_groups, T, d_out, in_group=3)
    refused(Status.ERR_INVALID, ["bank_process_listed_groups", "streamed input"], bank.process_listed_groups, T, d_out, in_group=4)
    refused(Status.ERR_INVALID, ["bank_process_listed_groups", "broadcast"], bank.process_listed_groups, T, d_out, Layout.QUAD, d_out, Layout.BROADCAST, 4)
    refused(Status.ERR_INVALID, ["bank_process_listed_groups", "null"], bank.process_listed_groups, T, 0)
    refused(Status.ERR_INVALID, ["bank_process_listed_groups", "aligned"], bank.process_listed_groups, T, d_out.ptr + 4)
    refused(Status.ERR_INVALID, ["bank_process_listed_groups", "layout"], bank.process_listed_groups, T, d_out, Layout.BROADCAST)
    refused(Status.ERR_INVALID, ["bank_process_listed_groups", "layout"], bank.process_listed_groups, T, d_out, Layout.QUAD, d_out, 7)
    refused(Status.ERR_INVALID, ["bank_process_listed_groups", "gains"], bank.process_listed_groups, T, d_out, d_gains=d_out.ptr + 2)
    refused(Status.ERR_INVALID, ["bank_process_listed_groups", "peaks"], bank.process_listed_groups, T, d_out, d_peak=d_out.ptr + 2)
    untouched(bank, st0, "bad arguments")
    with eng.record():
        refused(Status.ERR_INVALID, ["bank_process_listed_groups", "recording", "contents"], bank.process_listed_groups, T, d_out)
    untouched(bank, st0, "while recording a sequence")
    bank.set_voice_list([])
    assert bank.listed_groups.size == 0 and bank.voice_list_size == 0
    bank.process_listed_groups(T, d_out)              # launches nothing
    untouched(bank, st0, "the empty list")
    bank.close()

    odd = eng.bank([Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN], 72)   # 72 voices: whole groups of 8, not of 16
    odd.reserve_voice_list_groups(8, 16)
    odd.set_voice_list([1, 5, 63])
    st = odd.get_all_state()
    refused(Status.ERR_INVALID, ["bank_process_listed_groups", "whole number"], odd.process_listed_groups, 1, d_out)
    untouched(odd, st, "voices that are not whole groups")
    odd.close()

    cascade = eng.bank([Proc.LOPASS, Proc.LOPASS], 64)
    assert cascade.fused and "cascade" in cascade.kernel_name
    eng.set_jit(False)
    try:
        unfused = eng.bank([Proc.NOISE_GEN, Proc.ONE_POLE], 64)
    finally:
        eng.set_jit(True)
    assert not unfused.fused
    scratch = eng.alloc(4 * 64 * 64)
    for b in (cascade, unfused):
        b.process(1, scratch)
        b.reserve_voice_list_groups(8, 16)
        b.set_voice_list([1, 5, 63])
        st = b.get_all_state()
        refused(Status.ERR_UNSUPPORTED, ["bank_process_listed_groups", "ahead-of-time"], b.process_listed_groups, 1, d_out)
        untouched(b, st, "an unsupported bank")
        b.close()
