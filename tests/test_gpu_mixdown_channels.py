"""The mixdown per channel on the device: mlgpu_bank_process_mixdown_channels, its listed and shard forms (chain_mix_channels_kernel,
chain_listed_mix_channels_kernel) and mlgpu_mixdown_channels - a stereo bus with a pan per voice, the voices advancing once.

Expected values come from the CPU checker alone (mixdown_channels_cases, voice_list_cases): chain_process per voice, then the checker's
mixdown(y, gains[c]) per channel. gains[0] = special_gains(V) (a -0.0, a 0.0 and a denormal among them), gains[1] its constant-power
partner sqrt(1 - g^2), one voice hard right (0.0 and exactly 1.0), one with a negative right gain. Every comparison is bit-exact."""
import numpy as np
import pytest

from bank_groups_cases import T
from inputs import assert_bits_equal
from madronalib_amd.constants import Layout, Proc, Status
from mixdown_channels_cases import C, SHAPES, SPLITS, case, channel_gains, expected_channels
from voice_list_cases import V as LV
from voice_list_cases import expected_listed, expected_listed_mixdown, expected_peaks, make_chain, voice_lists

GUARD = np.uint32(0x7FC5A5A5)   # what the memory around an output holds before a launch
LISTS = voice_lists()
_listed = {}


@pytest.fixture(scope="module")
def eng():
    import madronalib_amd as ml
    e = ml.Engine(0)
    e.mixdown_reserve_channels(8192, T, C)
    yield e
    e.set_flush_denormals(False)
    e.close()


def guarded(eng, words, guard_words):
    d = eng.alloc(4 * (words + guard_words))
    d.upload(np.full(words + guard_words, GUARD, np.uint32))
    return d


def fresh_bank(eng, ch, prelude=False):
    """The chain's bank from clear(); prelude: after one DSPVector of all its voices (what the listed cases start from)."""
    bank = eng.bank(ch.procs, ch.V)
    bank.clear()
    bank.set_all_coeffs(ch.coeffs)
    bank.set_input_const(ch.in_const)
    if prelude:
        bank.process(1, eng.alloc(4 * ch.V * 64), Layout.QUAD)
    return bank


def run_channels(eng, call, splits, rows=1):
    """call(n, d_out) over launches of `splits` DSPVectors, d_out [C][rows][64 n] with one guard row behind it that must come back
    untouched. Returns [C][rows][64 T]."""
    outs = []
    for n in splits:
        d_out = guarded(eng, C * rows * 64 * n, 64 * n)
        call(n, d_out)
        raw = d_out.download(np.uint32)
        assert (raw[C * rows * 64 * n:] == GUARD).all(), "the row behind d_out[C] was written"
        outs.append(raw[:C * rows * 64 * n].view(np.float32).reshape(C, rows, 64 * n))
    return np.concatenate(outs, 2)


def check_channels(eng, oracle, name, V, flush=False):
    ch, gains, y, want, st = case(oracle, name, V, flush)
    what = f"{name} V={V} flush={flush}"
    eng.set_flush_denormals(flush)
    try:
        d_gains = eng.to_device(gains)
        got, states = {}, {}
        for splits in SPLITS:
            bank = fresh_bank(eng, ch)
            got[splits] = run_channels(eng, lambda n, d: bank.process_mixdown_channels(n, C, d_gains, d), splits)[:, 0]
            states[splits] = bank.get_all_state()
            bank.close()
        # HIP against HIP: one one-channel call per channel, each on a fresh bank from the same state
        single = []
        for c in range(C):
            bank = fresh_bank(eng, ch)
            d_one = eng.alloc(4 * 64 * T)
            bank.process_mixdown(T, d_one, None, Layout.QUAD, d_gains.ptr + 4 * c * V)
            single.append(d_one.download(np.float32, 64 * T))
            single_state = bank.get_all_state()
            bank.close()
        # ... and the three calls it replaces: process into memory, then a mixdown per channel
        bank = fresh_bank(eng, ch)
        d_sig, d_three = eng.alloc(4 * V * 64 * T), guarded(eng, C * 64 * T, 64 * T)
        bank.process(T, d_sig, Layout.QUAD)
        eng.mixdown_channels(d_sig, Layout.QUAD, V, T, C, d_gains, d_three)
        three = d_three.download(np.uint32)
        bank.close()
    finally:
        eng.set_flush_denormals(False)
    one = got[SPLITS[0]]
    assert np.isfinite(want).all() and np.abs(want).max() > 1e-6, what
    for c in range(C):
        assert_bits_equal(one[c], want[c], True, f"{what}: channel {c} of one launch against the oracle's voices and tree")
        assert_bits_equal(got[SPLITS[1]][c], one[c], True, f"{what}: channel {c}, launches of 1 + 2 against one launch")
        assert_bits_equal(one[c], single[c], True, f"{what}: channel {c} against process_mixdown with that channel's gains (HIP against HIP)")
    assert (three[C * 64 * T:] == GUARD).all(), "mixdown_channels wrote behind d_out[C]"
    assert_bits_equal(one, three[:C * 64 * T].view(np.float32).reshape(C, 64 * T), True, what + ": against process -> mixdown_channels")
    assert_bits_equal(states[SPLITS[0]], st, False, what + ": state against the oracle (the voices advanced once)")
    assert_bits_equal(states[SPLITS[1]], states[SPLITS[0]], False, what + ": state after 1 + 2 against one launch")
    assert_bits_equal(single_state, states[SPLITS[0]], False, what + ": state against the one-channel call's")


@pytest.mark.gpu
@pytest.mark.parametrize("V,name", SHAPES)
def test_two_channels_have_the_bits_of_two_one_channel_calls(eng, oracle, V, name):
    """SawGen -> Bandpass -> Gain, T = 3, one launch of 3 and launches of 1 + 2. V = 80 (a wavefront and a quarter: spare lanes in the
    tree), 2352 (nine workgroups through the XCD remap and a last one of 48 voices), 4160 (65 first-stage groups: each channel's region
    goes through two levels of the tree); saw_odd mixes head modes in the first and last wavefront. Each channel against the oracle,
    against process_mixdown with that channel's gains on a fresh bank, against process + mixdown_channels; the state against the
    oracle's after ONE run; the guard row behind d_out[C]."""
    check_channels(eng, oracle, name, V)


@pytest.mark.gpu
@pytest.mark.parametrize("flush", [pytest.param(False, id="ieee"), pytest.param(True, id="flush")])
@pytest.mark.parametrize("V", [80, 2352])
def test_two_channels_in_both_float_modes(eng, oracle, V, flush):
    check_channels(eng, oracle, "saw_odd", V, flush=flush)


@pytest.mark.gpu
def test_one_channel_is_the_one_channel_call(eng, oracle):
    ch, gains, y, want, st = case(oracle, "saw", 80)
    d_gains = eng.to_device(gains)
    outs = []
    for chan in (True, False):
        bank = fresh_bank(eng, ch)
        d_out = guarded(eng, 64 * T, 64 * T)
        if chan:
            bank.process_mixdown_channels(T, 1, d_gains, d_out)
        else:
            bank.process_mixdown(T, d_out, None, Layout.QUAD, d_gains)
        outs.append(d_out.download(np.uint32))
        bank.close()
    assert_bits_equal(outs[0], outs[1], False, "n_channels = 1 against process_mixdown, guard row included")
    assert_bits_equal(outs[0][:64 * T].view(np.float32), want[0], True, "n_channels = 1 against the oracle")
    bank = fresh_bank(eng, ch)
    d_out = eng.alloc(4 * 64 * T)
    bank.process_mixdown_channels(T, 1, None, d_out)     # (one channel: the gains may be null, as today)
    assert_bits_equal(d_out.download(np.float32, 64 * T), oracle.mixdown(y, None), True, "n_channels = 1 without gains")
    bank.close()


def listed_case(oracle, name, lname):
    """(chain, state after the prelude, the listed voices' signals [K][64 T], the full state after) as test_gpu_voice_list has them."""
    key = (name, lname)
    if key not in _listed:
        if ("chain", name) not in _listed:
            ch = make_chain(oracle, name)
            st0 = oracle.chain_clear(ch.procs, LV)
            oracle.chain_process(ch.procs, 1, ch.coeffs, st0, None, ch.in_const, n_threads=4, want_out=False)
            st0.setflags(write=False)
            _listed[("chain", name)] = (ch, st0)
        ch, st0 = _listed[("chain", name)]
        st = st0.copy()
        y = expected_listed(oracle, ch, LISTS[lname], st, 0, T)
        y.setflags(write=False), st.setflags(write=False)
        _listed[key] = (ch, st0, y, st)
    return _listed[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name,lname", [("saw", l) for l in ("last", "k80", "k2100", "all", "empty")] + [("saw_odd", "k80")])
def test_listed_two_channels(eng, oracle, name, lname):
    """process_listed_mixdown_channels on V = 2352: K = 1, 80 (spare lanes), 2100 (nine workgroups), V and 0. Every bank first runs one
    DSPVector on all voices. The gains are gathered by VOICE (channel stride V, not K); the peaks are taken before any gain; the
    unlisted voices' state stays; an empty list gives +0.0 in both channels; the list of all voices gives the bits of the unlisted call."""
    ch, st0, y, st = listed_case(oracle, name, lname)
    L = LISTS[lname]
    K = L.size
    gains = channel_gains(LV)
    want = np.stack([expected_listed_mixdown(oracle, y, L, gains[c]) for c in range(C)])
    what = f"{name} list={lname} K={K}"
    d_gains = eng.to_device(gains)
    got, states, peaks = {}, {}, {}
    for splits in SPLITS:
        bank = fresh_bank(eng, ch, prelude=True)
        bank.set_voice_list(L)
        if splits == SPLITS[0]:
            assert_bits_equal(bank.get_all_state(), st0, False, what + ": state before the call against the oracle")
        pk = []

        def call(n, d_out):
            d_peak = guarded(eng, K, 1)
            bank.process_listed_mixdown_channels(n, C, d_gains, d_out, d_peak=d_peak)
            raw = d_peak.download(np.uint32)
            assert raw[K] == GUARD, "the word behind d_peak[K] was written"
            pk.append(raw[:K].copy())
        got[splits] = run_channels(eng, call, splits)[:, 0]
        states[splits], peaks[splits] = bank.get_all_state(), pk
        bank.close()
    if K == LV:
        bank = fresh_bank(eng, ch, prelude=True)
        unlisted = run_channels(eng, lambda n, d: bank.process_mixdown_channels(n, C, d_gains, d), SPLITS[0])[:, 0]
        unlisted_state = bank.get_all_state()
        bank.close()
    one = got[SPLITS[0]]
    if K:
        assert np.isfinite(want).all() and np.abs(want).max() > 1e-6 and (want[0].view(np.uint32) != want[1].view(np.uint32)).any(), what
    else:
        assert (want.view(np.uint32) == 0).all() and (one.view(np.uint32) == 0).all(), what + ": +0.0 in every channel"
    for c in range(C):
        assert_bits_equal(one[c], want[c], True, f"{what}: channel {c} against the oracle's voices and tree")
        assert_bits_equal(got[SPLITS[1]][c], one[c], True, f"{what}: channel {c}, launches of 1 + 2 against one launch")
    for splits in SPLITS:
        t0 = 0
        for pk, n in zip(peaks[splits], splits):
            assert_bits_equal(pk, expected_peaks(y[:, 64 * t0:64 * (t0 + n)]), False, f"{what}: peaks (before any gain) of DSPVectors {t0}..{t0 + n - 1}")
            t0 += n
    assert_bits_equal(states[SPLITS[0]], st, False, what + ": state against the oracle (listed voices advanced once, the others where they were)")
    assert_bits_equal(states[SPLITS[1]], states[SPLITS[0]], False, what + ": state after 1 + 2 against one launch")
    if K == LV:
        assert_bits_equal(one, unlisted, True, what + ": against process_mixdown_channels of a second bank")
        assert_bits_equal(states[SPLITS[0]], unlisted_state, False, what + ": state against process_mixdown_channels of a second bank")


@pytest.mark.gpu
def test_two_shards_finish_to_one_engines_channels(eng, oracle):
    """V = 8192 as two shards of 4096 voices, banks of one engine: each channel's rows of both shards, finished by mixdown_finish,
    are the one-bank channel; that against the oracle's voices and tree."""
    import madronalib_amd as ml
    ch, gains, y, want, st = case(oracle, "saw", 8192)
    V, per = 8192, 4096
    nrows = ml.mixdown_shard_rows(per)
    assert ml.mixdown_shard_level(per) == 2 and nrows == 1
    whole = fresh_bank(eng, ch)
    d_gains = eng.to_device(gains)
    one = run_channels(eng, lambda n, d: whole.process_mixdown_channels(n, C, d_gains, d), SPLITS[0])[:, 0]
    assert_bits_equal(whole.get_all_state(), st, False, "state of the one bank against the oracle")
    whole.close()
    rows = []
    for k in range(2):
        part = eng.bank(ch.procs, per)
        part.clear()
        part.set_all_coeffs(np.ascontiguousarray(ch.coeffs[:, k * per:(k + 1) * per]))
        part.set_input_const(np.ascontiguousarray(ch.in_const[k * per:(k + 1) * per]))
        d_g = eng.to_device(np.ascontiguousarray(gains[:, k * per:(k + 1) * per]))
        rows.append(run_channels(eng, lambda n, d: part.process_mixdown_channels_shard(n, C, d_g, d), SPLITS[0], rows=nrows))
        assert_bits_equal(part.get_all_state(), st[:, k * per:(k + 1) * per], False, f"state of shard {k} against the oracle")
        part.close()
    for c in range(C):
        assert_bits_equal(one[c], want[c], True, f"channel {c} of the one bank against the oracle")
        finished = ml.mixdown_finish(np.ascontiguousarray(np.concatenate([r[c] for r in rows], 0)))
        assert_bits_equal(finished, one[c], True, f"channel {c}: two shards finished on the host against the one bank")


def refused(status, words, fn, *args, **kw):
    import madronalib_amd as ml
    with pytest.raises(ml.MlgpuError) as ei:
        fn(*args, **kw)
    assert ei.value.status == status, str(ei.value)
    assert all(w in str(ei.value) for w in words), str(ei.value)


@pytest.mark.gpu
def test_refusals(eng, oracle):
    """n_channels other than 1 or 2: MLGPU_ERR_UNSUPPORTED. Null gains, gains not 4-byte aligned, outputs not 16-byte aligned, a
    reservation that is too small (the message names the reserve call): MLGPU_ERR_INVALID. A bank without the ahead-of-time summing
    form - an SVF cascade, a bank served only through prepare_mixdown: MLGPU_ERR_UNSUPPORTED, the message names the three-call
    route. Every message starts with the call's name; a refused call leaves the state where it was."""
    import madronalib_amd as ml
    ch, gains, y, want, st = case(oracle, "saw", 80)
    V = 80
    bank = fresh_bank(eng, ch)
    bank.set_voice_list([1, 5, 63])
    st0 = bank.get_all_state()
    d_gains, d_out, d_sig = eng.to_device(gains), eng.alloc(4 * C * 64 * T), eng.alloc(4 * V * 64 * T)
    calls = {
        "bank_process_mixdown_channels": lambda n_ch, g, out: bank.process_mixdown_channels(T, n_ch, g, out),
        "bank_process_mixdown_channels_shard": lambda n_ch, g, out: bank.process_mixdown_channels_shard(T, n_ch, g, out),
        "bank_process_listed_mixdown_channels": lambda n_ch, g, out: bank.process_listed_mixdown_channels(T, n_ch, g, out),
        "mixdown_channels": lambda n_ch, g, out: eng.mixdown_channels(d_sig, Layout.QUAD, V, T, n_ch, g, out),
    }
    for name, call in calls.items():
        for n_ch in (0, 3, -1):
            refused(Status.ERR_UNSUPPORTED, [name, "channels"], call, n_ch, d_gains, d_out)
        refused(Status.ERR_INVALID, [name, "null gains"], call, C, None, d_out)
        refused(Status.ERR_INVALID, [name, "gains"], call, C, d_gains.ptr + 2, d_out)
        refused(Status.ERR_INVALID, [name, "aligned"], call, C, d_gains, d_out.ptr + 4)
        refused(Status.ERR_INVALID, [name, "null"], call, C, d_gains, 0)
    refused(Status.ERR_INVALID, ["bank_process_mixdown_channels_shard", "multiple of 64"], calls["bank_process_mixdown_channels_shard"], C, d_gains, d_out)
    assert_bits_equal(bank.get_all_state(), st0, False, "state after refused calls")
    bank.close()

    # a reservation that is too small: none at all, one channel's worth, then enough
    small = ml.Engine(0)
    b = small.bank(ch.procs, 8192)
    b.set_voice_list(np.arange(0, 8192, 2))
    g8, out8, sig8 = small.alloc(4 * C * 8192), small.alloc(4 * C * 64), small.alloc(4 * 8192 * 64)
    for reserve in (None, lambda: small.mixdown_reserve(8192, 1), lambda: small.mixdown_reserve_channels(8192, 1, 1)):
        if reserve:
            reserve()
        refused(Status.ERR_INVALID, ["bank_process_mixdown_channels", "mlgpu_mixdown_reserve_channels"], b.process_mixdown_channels, 1, C, g8, out8)
        refused(Status.ERR_INVALID, ["bank_process_mixdown_channels_shard", "mlgpu_mixdown_reserve_channels"], b.process_mixdown_channels_shard, 1, C, g8, out8)
        refused(Status.ERR_INVALID, ["mixdown_channels", "mlgpu_mixdown_reserve_channels"], small.mixdown_channels, sig8, Layout.QUAD, 8192, 1, C, g8, out8)
    small.mixdown_reserve_channels(4096, 1, C)
    b.process_listed_mixdown_channels(1, C, g8, out8)      # (4096 listed voices: enough)
    refused(Status.ERR_INVALID, ["bank_process_mixdown_channels", "mlgpu_mixdown_reserve_channels"], b.process_mixdown_channels, 1, C, g8, out8)
    small.mixdown_reserve_channels(8192, 1, C)
    b.process_mixdown_channels(1, C, g8, out8)
    refused(Status.ERR_INVALID, ["mixdown_reserve_channels", "channel"], small.mixdown_reserve_channels, 64, 1, 0)
    small.close()

    # banks without the ahead-of-time summing form
    cascade = eng.bank([Proc.LOPASS, Proc.LOPASS], 64)
    assert cascade.fused and "cascade" in cascade.kernel_name
    generated = eng.bank([Proc.NOISE_GEN, Proc.ONE_POLE], 64)
    generated.prepare_mixdown()
    generated.process_mixdown(1, d_out)                    # (the one-channel call serves it)
    g64 = eng.alloc(4 * C * 64)
    for b in (cascade, generated):
        b.set_voice_list([1, 5, 63])
        before = b.get_all_state()
        for name in ("process_mixdown_channels", "process_mixdown_channels_shard", "process_listed_mixdown_channels"):
            refused(Status.ERR_UNSUPPORTED, ["bank_" + name, "ahead-of-time", "mlgpu_bank_process", "mlgpu_mixdown_channels"], getattr(b, name), 1, C, g64, d_out)
        assert_bits_equal(b.get_all_state(), before, False, "state after an unsupported call")
        b.close()
