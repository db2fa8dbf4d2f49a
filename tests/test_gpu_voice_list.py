"""Voice lists on the device: mlgpu_bank_set_voice_list, mlgpu_bank_process_listed and _listed_mixdown (chain_listed_kernel,
chain_listed_mix_kernel) - a listed call behaves as a bank of K voices made of voices L[0] ... L[K-1], and nobody else is touched.

Expected values (voice_list_cases): the CPU checker's chain_process on the K listed voices - coefficients, input constant and input
rows gathered by L, the state rows taken from and scattered back into the full bank's state -, the checker's mixdown of those rows
with the gains gathered by L, the peaks in numpy on the expected output's bits. Every bank first runs one DSPVector on ALL its voices
(and so does the checker), so that the state an unlisted voice must keep is not the cleared one. All comparisons are bit-exact."""
import types

import numpy as np
import pytest

from bank_groups_cases import T, special_gains
from inputs import assert_bits_equal
from madronalib_amd.constants import Layout, Proc, Status
from voice_list_cases import V, chain_inputs, expected_listed, expected_listed_mixdown, expected_peaks, make_chain, voice_lists

GUARD = np.uint32(0x7FC5A5A5)   # what the memory around an output holds before a launch
LISTS = voice_lists()
_prepared, _expected = {}, {}


@pytest.fixture(scope="module")
def eng():
    import madronalib_amd as ml
    e = ml.Engine(0)
    e.mixdown_reserve(V, T)
    yield e
    e.set_flush_denormals(False)
    e.close()


def prepared(oracle, name, flush=False):
    """(chain, the checker's state after one DSPVector of all V voices from clear()), once per chain and mode, left unchanged."""
    key = (name, flush)
    if key not in _prepared:
        ch = make_chain(oracle, name)
        st0 = oracle.chain_clear(ch.procs, V)
        x = chain_inputs(ch)
        with oracle.flush_denormals(flush):
            oracle.chain_process(ch.procs, 1, ch.coeffs, st0, None if x is None else np.ascontiguousarray(x[:, :64]), ch.in_const, n_threads=4, want_out=False)
        st0.setflags(write=False)
        _prepared[key] = (ch, st0)
    return _prepared[key]


def reference(oracle, name, lname, flush=False):
    """(chain, state before, the listed voices' signals [K][64 T], the full state after) for one launch of T DSPVectors."""
    key = (name, lname, flush)
    if key not in _expected:
        ch, st0 = prepared(oracle, name, flush)
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


def make_bank(eng, ch, coeffs=None, in_const=None):
    """The chain's bank after one DSPVector of all its voices (the state `prepared` has)."""
    bank = eng.bank(ch.procs, ch.V)
    bank.clear()
    bank.set_all_coeffs(ch.coeffs if coeffs is None else coeffs)
    ic = ch.in_const if in_const is None else in_const
    if ic is not None:
        bank.set_input_const(ic)
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


def run_listed(eng, bank, ch, K, splits, out_layout=Layout.QUAD, in_layout=Layout.QUAD, mix=False, d_gains=None):
    """process_listed (mix: process_listed_mixdown) over launches of `splits` DSPVectors with the list the bank has. Every output has
    one guard row behind it, every d_peak[K] one guard word, that must come back untouched. Returns ([K][64 T], or [64 T] for the
    mixdown; the peaks [K] of each launch)."""
    x = chain_inputs(ch)
    outs, peaks, t0 = [], [], 0
    for n in splits:
        d_in = None if x is None else to_layout(eng, x[:, 64 * t0:64 * (t0 + n)], in_layout, n)
        rows = 1 if mix else K
        d_out = guarded(eng, rows * 64 * n, 64 * n)
        d_peak = guarded(eng, K, 1)
        if mix:
            bank.process_listed_mixdown(n, d_out, d_in, in_layout, d_gains, d_peak)
        else:
            bank.process_listed(n, d_out, out_layout, d_in, in_layout, d_peak)
        raw = d_out.download(np.uint32)
        assert (raw[rows * 64 * n:] == GUARD).all(), "the row behind the output was written"
        if mix or K == 0:
            outs.append(raw[:rows * 64 * n].view(np.float32).reshape(rows, 64 * n))
        else:
            d_vm = eng.alloc(4 * K * 64 * n)
            eng.layout_convert(d_out, out_layout, d_vm, Layout.VOICE_MAJOR, K, n)
            outs.append(d_vm.download(np.float32, K * 64 * n).reshape(K, 64 * n))
        pk = d_peak.download(np.uint32)
        assert pk[K] == GUARD, "the word behind d_peak[K] was written"
        peaks.append(pk[:K].copy())
        t0 += n
    out = np.concatenate(outs, 1)
    return (out[0] if mix else out), peaks


def check_peaks(peaks, y, splits, what):
    """The peaks of each launch are those of that launch's samples alone (written once per launch, not accumulated)."""
    t0 = 0
    for pk, n in zip(peaks, splits):
        assert_bits_equal(pk, expected_peaks(y[:, 64 * t0:64 * (t0 + n)]), False, f"{what}: peaks of the launch of DSPVectors {t0}..{t0 + n - 1}")
        t0 += n


def check_listed(eng, oracle, name, lname, flush=False, out_layout=Layout.QUAD, in_layout=Layout.QUAD):
    ch, st0, y, st = reference(oracle, name, lname, flush)
    L = LISTS[lname]
    K, rest = L.size, np.setdiff1d(np.arange(V), L)
    what = f"{name} list={lname} K={K} flush={flush} out={int(out_layout)} in={int(in_layout)}"
    eng.set_flush_denormals(flush)
    try:
        bank = make_bank(eng, ch)
        bank.set_voice_list(L)
        assert bank.voice_list_size == K
        before = (bank.get_all_state(), all_coeffs(bank), bank.get_input_const())
        one, peaks_one = run_listed(eng, bank, ch, K, [T], out_layout, in_layout)
        after = (bank.get_all_state(), all_coeffs(bank), bank.get_input_const())
        bank.set_all_state(before[0])
        split, peaks_split = run_listed(eng, bank, ch, K, [1, T - 1], out_layout, in_layout)
        state_split = bank.get_all_state()
        bank.close()
        if K == V:
            plain = make_bank(eng, ch)
            x = chain_inputs(ch)
            d_plain = eng.alloc(4 * V * 64 * T)
            plain.process(T, d_plain, Layout.VOICE_MAJOR, None if x is None else eng.to_device(x), Layout.VOICE_MAJOR)
            plain_out, plain_state = d_plain.download(np.float32).reshape(V, 64 * T), plain.get_all_state()
            plain.close()
    finally:
        eng.set_flush_denormals(False)
    assert_bits_equal(before[0], st0, False, what + ": state before the call against the oracle")
    if K:
        assert np.isfinite(y).all() and np.abs(y).max() > 1e-6, what
    assert_bits_equal(one, y, True, what + ": one launch against the oracle")
    assert_bits_equal(split, one, True, what + ": launches of 1 + 2 against one launch")
    check_peaks(peaks_one, y, [T], what)
    check_peaks(peaks_split, y, [1, T - 1], what + " (1 + 2)")
    assert_bits_equal(after[0][:, L], st[:, L], False, what + ": state of the listed voices against the oracle")
    assert_bits_equal(after[0][:, rest], before[0][:, rest], False, what + ": state of the unlisted voices against the download before the call")
    assert_bits_equal(after[1], before[1], False, what + ": coefficients against the download before the call")
    assert_bits_equal(after[2], before[2], False, what + ": input constants against the download before the call")
    assert_bits_equal(state_split, after[0], False, what + ": state after 1 + 2 against one launch")
    if K == V:
        assert_bits_equal(one, plain_out, True, what + ": against Bank.process of a second bank")
        assert_bits_equal(after[0], plain_state, False, what + ": state against Bank.process of a second bank")


ALL_LISTS = ("last", "wave", "k80", "k2100", "all", "empty")


@pytest.mark.gpu
@pytest.mark.parametrize("name,lname", [("saw", l) for l in ALL_LISTS] + [("saw_odd", l) for l in ("k80", "k2100", "all")] +
                         [("impulse", l) for l in ALL_LISTS])
def test_process_listed_on_a_constant_input(eng, oracle, name, lname):
    """SawGen -> Bandpass -> Gain with the fast head (saw) and with voices 5 and V - 3 - both listed - sending their wavefronts to the
    slow head (saw_odd), and ImpulseGen (its LDS table and workgroup barrier ahead of any lane's exit). V = 2352; K = 1 (the last
    voice), 64 (one wavefront, every 37th voice), 80 and 2100 (seeded random; nine workgroups, eight through the XCD remap, a last one
    of 52 lanes), V (against Bank.process of a second bank) and 0. One launch of 3 DSPVectors and launches of 1 + 2; output rows,
    guard row, peaks and their guard word, the listed voices' state against the oracle, every state, coefficient and input-constant
    word of the unlisted voices against a download taken before the call."""
    check_listed(eng, oracle, name, lname)


@pytest.mark.gpu
@pytest.mark.parametrize("lname,out_layout,in_layout", [(l, Layout.QUAD, Layout.QUAD) for l in ALL_LISTS] +
                         [(l, Layout.VOICE_MAJOR, Layout.VOICE_MAJOR) for l in ("last", "k80", "k2100", "all")] +
                         [("k80", Layout.ROWS, Layout.ROWS), ("k2100", Layout.QUAD, Layout.VOICE_MAJOR)])
def test_process_listed_gathers_a_streamed_input(eng, oracle, lname, out_layout, in_layout):
    """Bandpass on a streamed input of V rows: lane i reads row L[i] of it (QUAD, VOICE_MAJOR, ROWS) and writes row i of a K-row
    output."""
    check_listed(eng, oracle, "bandpass", lname, out_layout=out_layout, in_layout=in_layout)


@pytest.mark.gpu
def test_process_listed_reads_a_broadcast_row_as_process_does(eng, oracle):
    """MLGPU_LAYOUT_BROADCAST: one row for every voice, listed or not - the same bits as that row given per voice."""
    ch, _ = prepared(oracle, "bandpass")
    L = LISTS["k80"]
    x = chain_inputs(ch)
    row = np.ascontiguousarray(x[3])
    outs = []
    for d_in, layout in ((eng.to_device(row), Layout.BROADCAST), (eng.to_device(np.ascontiguousarray(np.repeat(row[None, :], V, axis=0))), Layout.VOICE_MAJOR)):
        bank = make_bank(eng, ch)
        bank.set_voice_list(L)
        d_out = eng.alloc(4 * L.size * 64 * T)
        bank.process_listed(T, d_out, Layout.VOICE_MAJOR, d_in, layout)
        outs.append(d_out.download(np.float32))
        bank.close()
    assert_bits_equal(outs[0], outs[1], True, "a broadcast input against the same row per voice")
    assert np.abs(outs[0]).max() > 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("flush", [pytest.param(False, id="ieee"), pytest.param(True, id="flush")])
@pytest.mark.parametrize("lname", ["k80", "k2100"])
def test_process_listed_in_both_float_modes(eng, oracle, lname, flush):
    check_listed(eng, oracle, "saw_odd", lname, flush=flush)


def check_mixdown(eng, oracle, name, lname, with_gains, flush=False):
    ch, st0, y, st = reference(oracle, name, lname, flush)
    L = LISTS[lname]
    K = L.size
    gains = special_gains(V) if with_gains else None
    want = expected_listed_mixdown(oracle, y, L, gains, flush)
    what = f"{name} list={lname} K={K} gains={with_gains} flush={flush}"
    eng.set_flush_denormals(flush)
    try:
        d_gains = None if gains is None else eng.to_device(gains)
        bank = make_bank(eng, ch)
        bank.set_voice_list(L)
        one, peaks_one = run_listed(eng, bank, ch, K, [T], mix=True, d_gains=d_gains)
        state_one = bank.get_all_state()
        bank.set_all_state(st0)
        split, peaks_split = run_listed(eng, bank, ch, K, [1, T - 1], mix=True, d_gains=d_gains)
        state_split = bank.get_all_state()
        bank.close()
        # the two calls it replaces, on the device: process_listed of a second bank, then mixdown of its K rows with the gains of
        # the listed voices
        hip = np.zeros(64 * T, np.float32)
        if K:
            two = make_bank(eng, ch)
            two.set_voice_list(L)
            d_rows, d_two = eng.alloc(4 * K * 64 * T), eng.alloc(4 * 64 * T)
            two.process_listed(T, d_rows, Layout.QUAD)
            eng.mixdown(d_rows, Layout.QUAD, K, T, d_two, None if gains is None else eng.to_device(np.ascontiguousarray(gains[L.astype(np.int64)])))
            hip = d_two.download(np.float32, 64 * T)
            two.close()
        if K == V:
            plain = make_bank(eng, ch)
            d_plain = eng.alloc(4 * 64 * T)
            plain.process_mixdown(T, d_plain, None, Layout.QUAD, d_gains)
            plain_out, plain_state = d_plain.download(np.float32, 64 * T), plain.get_all_state()
            plain.close()
    finally:
        eng.set_flush_denormals(False)
    if K:
        assert np.isfinite(want).all() and np.abs(want).max() > 1e-6, what
    else:
        assert (want.view(np.uint32) == 0).all()
    assert_bits_equal(one, want, True, what + ": one launch against the oracle's voices and tree")
    assert_bits_equal(split, one, True, what + ": launches of 1 + 2 against one launch")
    assert_bits_equal(one, hip, True, what + ": against process_listed -> mixdown (HIP against HIP)")
    check_peaks(peaks_one, y, [T], what)          # (the voice's own sample: before the gain)
    check_peaks(peaks_split, y, [1, T - 1], what + " (1 + 2)")
    assert_bits_equal(state_one, st, False, what + ": state against the oracle (listed voices advanced, the others where they were)")
    assert_bits_equal(state_split, state_one, False, what + ": state after 1 + 2 against one launch")
    if K == V:
        assert_bits_equal(one, plain_out, True, what + ": against Bank.process_mixdown of a second bank")
        assert_bits_equal(state_one, plain_state, False, what + ": state against Bank.process_mixdown of a second bank")


@pytest.mark.gpu
@pytest.mark.parametrize("with_gains", [pytest.param(False, id="plain"), pytest.param(True, id="gains")])
@pytest.mark.parametrize("name,lname", [("saw", l) for l in ALL_LISTS] + [("saw_odd", l) for l in ("k80", "k2100", "all")])
def test_process_listed_mixdown(eng, oracle, name, lname, with_gains):
    """The mixdown tree of a K-voice bank over the list positions - pairwise inside 64 consecutive positions (the spare lanes of a last
    wavefront that is not full run the list's last voice again and add +0), then mlgpu_mixdown's later stages - with and without
    per-voice gains (special_gains: a -0.0, a 0.0 and a denormal among them), indexed by VOICE. d_out has the bits of the oracle's
    voices under the oracle's tree, and the bits of Engine.mixdown applied to process_listed's output on the device: that second
    comparison is HIP against HIP, one step removed from the oracle. State as in the process_listed tests; an empty list gives +0.0;
    K = V gives Bank.process_mixdown's bits."""
    check_mixdown(eng, oracle, name, lname, with_gains)


@pytest.mark.gpu
@pytest.mark.parametrize("flush", [pytest.param(False, id="ieee"), pytest.param(True, id="flush")])
def test_process_listed_mixdown_in_both_float_modes(eng, oracle, flush):
    check_mixdown(eng, oracle, "saw_odd", "k80", True, flush=flush)


@pytest.mark.gpu
@pytest.mark.parametrize("with_gains", [pytest.param(False, id="plain"), pytest.param(True, id="gains")])
def test_process_listed_mixdown_on_a_streamed_frequency(eng, oracle, with_gains):
    """The listed summing form with a streamed input (the cases above give SawGen -> Bandpass -> Gain its frequency as a per-voice
    constant): the frequency as a signal of V rows, lane i reading row L[i]. V = 64 * 2 + 37, T = 3, every voice listed but 7, 64 and
    150 - K = 162, two wavefronts and 34 lanes, so the last wavefront has spare lanes. The sum against the oracle's voices under the
    oracle's tree, the peaks, the listed voices' state against the oracle and the unlisted voices' against a download before the call."""
    Vs = 64 * 2 + 37
    ch = make_chain(oracle, "saw", Vs)
    wobble = 1.0 + 0.3 * np.sin(np.arange(64 * T)[None, :] * 0.003 * (1 + np.arange(Vs)[:, None] % 7))
    ch.in_rows, ch.in_const = np.ascontiguousarray((ch.in_const[:, None] * wobble).astype(np.float32)), None
    rest = np.array([7, 64, 150])
    L = np.setdiff1d(np.arange(Vs), rest).astype(np.uint32)
    K = L.size
    st0 = oracle.chain_clear(ch.procs, Vs)
    oracle.chain_process(ch.procs, 1, ch.coeffs, st0, np.ascontiguousarray(ch.in_rows[:, :64]), None, n_threads=4, want_out=False)   # (make_bank's DSPVector)
    st = st0.copy()
    y = expected_listed(oracle, ch, L, st, 0, T)
    gains = special_gains(Vs) if with_gains else None
    want = expected_listed_mixdown(oracle, y, L, gains)
    bank = make_bank(eng, ch)
    bank.set_voice_list(L)
    before = bank.get_all_state()
    got, peaks = run_listed(eng, bank, ch, K, [T], mix=True, d_gains=None if gains is None else eng.to_device(gains))
    after = bank.get_all_state()
    bank.close()
    assert np.isfinite(want).all() and np.abs(want).max() > 1e-6
    assert_bits_equal(before, st0, False, "state before the call against the oracle")
    assert_bits_equal(got, want, True, "one launch against the oracle's voices and tree")
    check_peaks(peaks, y, [T], "streamed frequency")
    assert_bits_equal(after[:, L], st[:, L], False, "state of the listed voices against the oracle")
    assert_bits_equal(after[:, rest], before[:, rest], False, "state of the unlisted voices against the download before the call")


@pytest.mark.gpu
def test_peaks_show_a_nan_and_a_silent_voice(eng, oracle):
    """d_peak[i] = max over the launch of bits(y) & 0x7fffffff as an unsigned integer, y the voice's own sample.
    A Gain bank (y = input constant * gain): the voice given a NaN input constant reports a value above 0x7f800000, the voice whose
    gain coefficient is 0 reports 0, every other voice the numpy value; the word behind d_peak[K] stays.
    SawGen -> Bandpass -> Gain in both forms (process_listed, process_listed_mixdown with gains): a voice whose Gain coefficient is 0
    reports 0 and every finite voice the numpy value of its sample BEFORE the mixdown gain. An oscillator head turns its frequency
    into a phase increment and a NaN frequency does not reach the output, so there the NaN voice is one with a NaN Gain coefficient.
    The NaN voice is held to the threshold, not to the oracle's bits: NaN payloads are not portable (inputs.assert_bits_equal)."""
    L = LISTS["k80"]
    Li = L.astype(np.int64)
    nan_pos, silent_pos = 3, 70        # list positions: in the first wavefront and in the last, partial one
    rng = np.random.default_rng(5)
    gain = types.SimpleNamespace(name="gain", V=V, in_group=1, procs=[Proc.GAIN], in_rows=None,
                                 coeffs=rng.uniform(0.1, 1.0, (1, V)).astype(np.float32), in_const=rng.uniform(-1, 1, V).astype(np.float32))
    gain.in_const[Li[nan_pos]] = np.float32(np.nan)
    gain.coeffs[0, Li[silent_pos]] = np.float32(0.0)
    saw, _ = prepared(oracle, "saw")
    saw_coeffs = saw.coeffs.copy()
    saw_coeffs[3, Li[nan_pos]] = np.float32(np.nan)
    saw_coeffs[3, Li[silent_pos]] = np.float32(0.0)
    finite = np.ones(L.size, bool)
    finite[nan_pos] = False

    def check(peaks, y, what):
        want = expected_peaks(y)
        assert want[silent_pos] == 0 and (want[finite] < 0x7F800000).all() and (want[finite & (np.arange(L.size) != silent_pos)] > 0).all()
        assert_bits_equal(peaks[finite], want[finite], False, what + ": peaks against numpy")
        assert peaks[silent_pos] == 0, what
        assert peaks[nan_pos] > 0x7F800000, f"{what}: the NaN voice reports 0x{int(peaks[nan_pos]):08x}"

    bank = eng.bank(gain.procs, V)
    bank.set_all_coeffs(gain.coeffs)
    bank.set_input_const(gain.in_const)
    bank.set_voice_list(L)
    _, peaks = run_listed(eng, bank, gain, L.size, [T])
    bank.close()
    st = oracle.chain_clear(gain.procs, V)
    check(peaks[0], expected_listed(oracle, gain, L, st), "Gain on a NaN input constant")

    st = oracle.chain_clear(saw.procs, V)
    y = expected_listed(oracle, saw, L, st, coeffs=saw_coeffs)
    d_gains = eng.to_device(special_gains(V))
    for mix in (False, True):
        bank = eng.bank(saw.procs, V)
        bank.clear()
        bank.set_all_coeffs(saw_coeffs)
        bank.set_input_const(saw.in_const)
        bank.set_voice_list(L)
        _, peaks = run_listed(eng, bank, saw, L.size, [T], mix=mix, d_gains=d_gains if mix else None)
        bank.close()
        check(peaks[0], y, "SawGen -> Bandpass -> Gain, " + ("process_listed_mixdown with gains" if mix else "process_listed"))


@pytest.mark.gpu
def test_lists_updates_and_process_calls_are_ordered_on_the_stream(eng, oracle):
    """set_voice_list(A), process, apply_updates(CLEAR of a voice in B but not in A), set_voice_list(B), process, set_voice_list(C),
    process - one DSPVector each, nothing waited for in between. A, B and C overlap and have different lengths, all within the reserve.
    Each block's output, and the final state of every voice, equal the oracle run over exactly the blocks the voice was listed in
    (and the clear in its place); the third set in a row is the one that waits for its call before last."""
    import madronalib_amd as ml
    ch, st0 = prepared(oracle, "saw")
    rng = np.random.default_rng(17)
    A = np.sort(rng.choice(V, 100, replace=False)).astype(np.uint32)
    stolen = int(np.setdiff1d(np.arange(V), A)[1234])
    B = np.sort(np.concatenate([A[::3], [stolen], np.setdiff1d(np.arange(V), np.concatenate([A, [stolen]]))[5:400:11]])).astype(np.uint32)
    C = np.sort(np.concatenate([A[1::2], B[::2], np.arange(2300, V)])).astype(np.uint32)
    C = np.unique(C)
    assert len({A.size, B.size, C.size}) == 3 and stolen in B and stolen not in A and np.intersect1d(A, B).size and np.intersect1d(B, C).size
    bank = make_bank(eng, ch)
    bank.reserve_voice_list(max(A.size, B.size, C.size))
    bank.reserve_updates(64)
    lists = (A, B, C)
    d_outs = [eng.alloc(4 * l.size * 64) for l in lists]
    d_peaks = [eng.alloc(4 * l.size) for l in lists]
    clear = [ml.Update.clear(-1, stolen, 1)]
    bank.set_voice_list(A)
    bank.process_listed(1, d_outs[0], Layout.VOICE_MAJOR, d_peak=d_peaks[0])
    bank.apply_updates(clear)
    bank.set_voice_list(B)
    bank.process_listed(1, d_outs[1], Layout.VOICE_MAJOR, d_peak=d_peaks[1])
    bank.set_voice_list(C)
    bank.process_listed(1, d_outs[2], Layout.VOICE_MAJOR, d_peak=d_peaks[2])
    assert bank.voice_list_size == C.size
    got = [d.download(np.float32).reshape(l.size, 64) for d, l in zip(d_outs, lists)]
    got_peaks = [d.download(np.uint32) for d in d_peaks]
    state = bank.get_all_state()
    bank.close()

    st = st0.copy()
    cleared = oracle.chain_clear(ch.procs, V)
    assert (st[:, stolen] != cleared[:, stolen]).any()     # (the clear is visible)
    want = []
    for k, l in enumerate(lists):
        if k == 1:
            st[:, stolen] = cleared[:, stolen]
        want.append(expected_listed(oracle, ch, l, st, 0, 1))
    for k, name in enumerate("ABC"):
        assert_bits_equal(got[k], want[k], True, f"the block of list {name}")
        assert_bits_equal(got_peaks[k], expected_peaks(want[k]), False, f"the peaks of list {name}")
    assert_bits_equal(state, st, False, "final state: every voice advanced by exactly the blocks it was listed in")


def refused(status, words, fn, *args, **kw):
    import madronalib_amd as ml
    with pytest.raises(ml.MlgpuError) as ei:
        fn(*args, **kw)
    assert ei.value.status == status, str(ei.value)
    assert all(w in str(ei.value) for w in words), str(ei.value)


@pytest.mark.gpu
def test_banks_without_the_listed_form_are_refused_with_their_state_untouched(eng):
    """A processor-by-processor bank and an SVF cascade bank: MLGPU_ERR_UNSUPPORTED from both calls, nothing launched. A chain kernel
    without an ahead-of-time summing form (Bandpass alone): process_listed runs, process_listed_mixdown is unsupported.
    process_listed_mixdown on an engine without a mixdown reserve: MLGPU_ERR_INVALID."""
    import madronalib_amd as ml
    d_out = eng.alloc(4 * 64 * 64)
    cascade = eng.bank([Proc.LOPASS, Proc.LOPASS], 64)
    assert cascade.fused and "cascade" in cascade.kernel_name
    eng.set_jit(False)
    try:
        unfused = eng.bank([Proc.NOISE_GEN, Proc.ONE_POLE], 64)
    finally:
        eng.set_jit(True)
    assert not unfused.fused
    alone = eng.bank([Proc.BANDPASS], 64)
    for b in (cascade, unfused, alone):
        b.process(1, d_out)
        b.set_voice_list([1, 5, 63])
        st = b.get_all_state()
        if b is not alone:
            refused(Status.ERR_UNSUPPORTED, ["bank_process_listed", "ahead-of-time"], b.process_listed, 1, d_out)
        refused(Status.ERR_UNSUPPORTED, ["bank_process_listed_mixdown", "ahead-of-time"], b.process_listed_mixdown, 1, d_out)
        assert_bits_equal(b.get_all_state(), st, False, "state after an unsupported call")
    alone.process_listed(1, d_out)
    for b in (cascade, unfused, alone):
        b.close()
    small = ml.Engine(0)
    b = small.bank([Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN], 8192)
    b.set_voice_list(np.arange(0, 8192, 2))
    refused(Status.ERR_INVALID, ["bank_process_listed_mixdown", "mixdown_reserve"], b.process_listed_mixdown, 1, small.alloc(4 * 64))
    small.close()


@pytest.mark.gpu
def test_bad_arguments_and_a_refused_list_leave_the_previous_list_in_force(eng, oracle):
    """Lists that are not strictly ascending (MLGPU_ERR_INVALID, the position in the message), that name a voice the bank does not have
    or are longer than the reserve (MLGPU_ERR_RANGE): nothing is enqueued, the list set before stays - a following process_listed
    gives its result. Null, misaligned and badly laid out signals: MLGPU_ERR_INVALID."""
    ch, st0, y, st = reference(oracle, "saw", "k80")
    A = LISTS["k80"]
    bank = make_bank(eng, ch)
    bank.reserve_voice_list(100)
    bank.set_voice_list(A)
    refused(Status.ERR_INVALID, ["bank_set_voice_list", "ascending", "position 2"], bank.set_voice_list, [4, 9, 9, 12])
    refused(Status.ERR_INVALID, ["bank_set_voice_list", "ascending", "position 1"], bank.set_voice_list, [40, 9])
    refused(Status.ERR_RANGE, ["bank_set_voice_list", "position 3", str(V)], bank.set_voice_list, [0, 1, 2, V])
    refused(Status.ERR_RANGE, ["bank_set_voice_list", "reserved 100"], bank.set_voice_list, np.arange(101))
    assert bank.voice_list_size == A.size
    d_out = eng.alloc(4 * A.size * 64 * T)
    refused(Status.ERR_INVALID, ["bank_process_listed", "null"], bank.process_listed, T, 0)
    refused(Status.ERR_INVALID, ["bank_process_listed", "aligned"], bank.process_listed, T, d_out.ptr + 4)
    refused(Status.ERR_INVALID, ["bank_process_listed", "layout"], bank.process_listed, T, d_out, Layout.BROADCAST)
    refused(Status.ERR_INVALID, ["bank_process_listed", "layout"], bank.process_listed, T, d_out, Layout.QUAD, d_out, 7)
    refused(Status.ERR_INVALID, ["bank_process_listed", "peaks"], bank.process_listed, T, d_out, Layout.QUAD, None, Layout.QUAD, d_out.ptr + 2)
    refused(Status.ERR_INVALID, ["bank_process_listed_mixdown", "null"], bank.process_listed_mixdown, T, 0)
    assert_bits_equal(bank.get_all_state(), st0, False, "state after refused calls")
    bank.process_listed(T, d_out, Layout.VOICE_MAJOR)
    assert_bits_equal(d_out.download(np.float32).reshape(A.size, 64 * T), y, True, "the list set before the refused ones is in force")
    assert_bits_equal(bank.get_all_state(), st, False, "state")
    bank.set_voice_list([])
    assert bank.voice_list_size == 0
    bank.process_listed(T, d_out, Layout.VOICE_MAJOR)              # launches nothing
    assert_bits_equal(bank.get_all_state(), st, False, "state after a call with the empty list")
    bank.close()


@pytest.mark.gpu
def test_recorded_into_a_sequence(eng, oracle):
    """set_voice_list reads host memory and is refused while recording. process_listed is recorded; the replay reads whichever list
    is on the device when it runs: after the list's contents change at equal length, the replay gives what a direct call with the new
    list gives (output, peaks and state)."""
    ch, _ = prepared(oracle, "saw")
    A = LISTS["k80"]
    A2 = np.sort(np.random.default_rng(23).choice(V, A.size, replace=False)).astype(np.uint32)
    assert (A2 != A).any()
    banks = [make_bank(eng, ch), make_bank(eng, ch)]
    d_out, d_peak = eng.alloc(4 * A.size * 64), eng.alloc(4 * A.size)
    outs = [[], []]
    for l in (A, A2):
        banks[0].set_voice_list(l)
        banks[0].process_listed(1, d_out, Layout.QUAD, d_peak=d_peak)
        outs[0].append((d_out.download(np.float32), d_peak.download(np.uint32)))
    banks[1].reserve_voice_list(A.size)
    banks[1].set_voice_list(A)
    with eng.record() as seq:
        refused(Status.ERR_INVALID, ["bank_set_voice_list", "recording"], banks[1].set_voice_list, A2)
        banks[1].process_listed(1, d_out, Layout.QUAD, d_peak=d_peak)
    assert seq.num_nodes >= 1
    seq.launch()
    outs[1].append((d_out.download(np.float32), d_peak.download(np.uint32)))
    banks[1].set_voice_list(A2)
    seq.launch()
    outs[1].append((d_out.download(np.float32), d_peak.download(np.uint32)))
    for k in range(2):
        assert_bits_equal(outs[1][k][0], outs[0][k][0], True, f"replay {k}")
        assert_bits_equal(outs[1][k][1], outs[0][k][1], False, f"peaks of replay {k}")
    assert np.abs(outs[0][1][0]).max() > 1e-6 and (outs[0][0][0].view(np.uint32) != outs[0][1][0].view(np.uint32)).any()
    assert_bits_equal(banks[1].get_all_state(), banks[0].get_all_state(), False, "state after two replays")
    for b in banks:
        b.close()
