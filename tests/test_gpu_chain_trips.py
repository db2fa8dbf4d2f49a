"""chain_kernel's third head loop: a SawGen head on a launch-constant frequency, every lane of the wavefront inside (0, 1/16], makes its
samples in trips of 8 - the polyBLEP division and polynomials once per zone per trip (mldsp_procs.hpp: Proc<SAW_GEN>::trip_u,
Chain::next_head_trip; mldsp_kernels.hpp: kHeadTrip). Same operands through the same operations, so the same bits: every comparison
here is bit-exact, outputs and final state, against the CPU checker's chain_process.

V = 64 * 9 + 37 voices (a ragged last wavefront), T = 3 DSPVectors = 24 trips. One kind of frequency or start phase per wavefront, so
that one kind's fall-back cannot hide what another's recognition misses:
  a  regular: log-uniform in 1e-4 .. 0.03, one lane at exactly 1/16 (the limit: still trips)            wavefronts 0, 6, 9
  b  as a, one lane at nextafter(1/16, 1): the whole wavefront takes the fast per-sample loop           wavefront 1
  c  every lane above 1/16, up to 0.2: the fast per-sample loop                                         wavefront 2
  d  regular lanes and one each of 0, -0.01, 1e-30, 2^-65, 2^65, inf, nan: the general loop             wavefront 3
  e  regular frequencies, start phases on the knife edges (as test_oscillator_trips_on_the_knife_edges builds them: 0 .. 23 counter
     units after a wrap, 0 .. 16 * 23 units before one, 1 .. 37 samples into the launch): trips that fall back  wavefronts 4, 7
  f  regular frequencies, random start phases                                                           wavefronts 5, 8
What keeps the cases from passing through the fall-back is asserted on the CPU, from the integer phase counters, before the device is
touched (trip_facts)."""
import numpy as np
import pytest

from bank_groups_cases import special_gains
from inputs import assert_bits_equal, chain_coeffs
from madronalib_amd.constants import Layout, Proc
from test_gpu_parity import _run_gpu
from voice_list_cases import expected_peaks

pytestmark = pytest.mark.gpu

T = 3
V = 64 * 9 + 37
N = 8                      # samples per trip
KIND = "abcdefaefa"        # the kind of wavefront v // 64
SEED = 2024
SAW = [Proc.SAW_GEN]
SAW_BP_GAIN = [Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN]
CHAINS = [pytest.param(SAW, id="saw"), pytest.param(SAW_BP_GAIN, id="saw_bandpass_gain")]
# an ascending list whose wavefronts of 64 positions are: a (trips), c (fast), d (general), e (trips that fall back), a, and 20 lanes of a
LIST = np.concatenate([np.arange(64 * w, 64 * (w + 1)) for w in (0, 2, 3, 4, 6)] + [np.arange(V - 20, V)]).astype(np.uint32)

_cache = {}


def voices():
    """(freq [V] float32, start phase counters [V] uint32), once."""
    if "voices" not in _cache:
        rng = np.random.default_rng(SEED)
        wave, lane = np.arange(V) // 64, np.arange(V) % 64
        kind = np.array([KIND[w] for w in wave])
        freq = (1e-4 * (300.0 ** rng.random(V))).astype(np.float32)                       # 1e-4 .. 0.03
        sixteenth = np.float32(1.0 / 16.0)
        freq[(kind == "a") & (lane == 11)] = sixteenth
        freq[(kind == "b") & (lane == 11)] = sixteenth
        freq[(kind == "b") & (lane == 40)] = np.nextafter(sixteenth, np.float32(1.0))
        c = kind == "c"
        freq[c] = np.maximum(rng.uniform(1.0 / 16.0, 0.2, int(c.sum())).astype(np.float32), np.nextafter(sixteenth, np.float32(1.0)))
        odd = np.array([0.0, -0.01, 1e-30, 2.0 ** -65, 2.0 ** 64 * 2.0, np.inf, np.nan], np.float32)
        freq[64 * KIND.index("d") + 3 + 8 * np.arange(odd.size)] = odd
        om = rng.integers(0, 2 ** 32, V, dtype=np.uint64)
        istep = np.rint(freq[kind == "e"].astype(np.float64) * 2.0 ** 32).astype(np.uint64)
        v = np.arange(V, dtype=np.uint64)[kind == "e"]
        k, j = v % 37 + 1, (v // 8) % 24
        e = om[kind == "e"]
        e = np.where(v % 4 == 1, 2 ** 32 * 64 - k * istep + j, e)
        e = np.where(v % 4 == 3, 2 ** 32 * 64 - k * istep - 16 * j, e)
        om[kind == "e"] = e
        freq.setflags(write=False)
        phases = (om % (2 ** 32)).astype(np.uint32)
        phases.setflags(write=False)
        _cache["voices"] = (freq, phases)
        check_the_cases_reach_the_trip_loop_and_its_fall_back()      # (on the CPU, before anything is given to the device)
    return _cache["voices"]


def trip_facts():
    """From the integer phase counters alone (wavefronts of regular frequencies: kinds a, e, f): per wavefront and trip, whether some
    lane's smallest or largest phase of the trip is within 2^-22 of 0 or 1 (the trip falls back to the per-sample form); per lane,
    whether two samples of one trip straddle a wrap."""
    freq, phases = voices()
    kind = np.array([KIND[w] for w in np.arange(V) // 64])
    regular = np.isin(kind, ["a", "e", "f"])
    istep = np.zeros(V, np.uint64)
    istep[regular] = np.rint(freq[regular].astype(np.float64) * 2.0 ** 32).astype(np.uint64)
    n = np.arange(1, 64 * T + 1, dtype=np.uint64)
    counter = (phases.astype(np.uint64)[:, None] + n[None, :] * istep[:, None]) % (2 ** 32)            # [V][64 T], exact
    h = (counter >> np.uint64(1)).astype(np.int64).astype(np.float32).reshape(V, 8 * T, N)             # the phase times 2^31, as PhasorGen rounds it
    suspect_lane = (h.min(2) < np.float32(2.0 ** 9)) | (h.max(2) > np.float32((1.0 - 2.0 ** -22) * 2.0 ** 31))
    c = counter.reshape(V, 8 * T, N)
    wraps = (c[:, :, 1:] < c[:, :, :-1]).any(2)                                                          # [V][trips]
    suspect = {w: np.array([suspect_lane[64 * w:64 * (w + 1), t].any() for t in range(8 * T)]) for w in range(len(KIND)) if KIND[w] in "aef"}
    return kind, suspect, wraps


def check_the_cases_reach_the_trip_loop_and_its_fall_back():
    """The conditions on the inputs (no device involved; every test gets its inputs through voices(), which asserts them first): wavefronts of kinds a and f make at least 90 % of their trips without the
    fall-back, every wavefront of kind e has a trip that falls back, some lane of kind a has a trip that straddles a wrap; the
    frequencies of kinds a, e, f are inside (0, 1/16], kind b's and c's wavefronts are outside by one lane / by all."""
    freq, _ = voices()
    kind, suspect, wraps = trip_facts()
    sixteenth = np.float32(1.0 / 16.0)
    for k in "aef":
        assert ((freq[kind == k] > 0) & (freq[kind == k] <= sixteenth)).all()
    assert (freq[kind == "a"] == sixteenth).sum() == KIND.count("a")
    assert (freq[kind == "b"] > sixteenth).sum() == 1 and (freq[kind == "c"] > sixteenth).all() and freq[kind == "c"].max() <= 0.2
    quiet = np.concatenate([~suspect[w] for w in suspect if KIND[w] in "af"])
    assert quiet.mean() >= 0.9, quiet.mean()
    for w in suspect:
        if KIND[w] == "e":
            assert suspect[w].any(), w
    assert wraps[kind == "a"].any()
    for w in (0, 4):          # the list's wavefronts 0 and 4 are whole wavefronts of kind a: entirely regular
        assert KIND[int(LIST[64 * w]) // 64] == "a" and (np.diff(LIST[64 * w:64 * (w + 1)]) == 1).all()
    assert (np.diff(LIST.astype(np.int64)) > 0).all()


def test_the_cases_reach_the_trip_loop_and_its_fall_back():
    voices()
    check_the_cases_reach_the_trip_loop_and_its_fall_back()


def reference(oracle, procs, flush=False):
    """(coeffs, state before, the voices' signals [V][64 T], state after) of one launch of T DSPVectors, once per chain and mode."""
    key = (tuple(procs), flush)
    if key not in _cache:
        freq, phases = voices()
        co = chain_coeffs(oracle, procs, V, seed=1)
        st0 = oracle.chain_clear(procs, V)
        st0[0] = phases
        st = st0.copy()
        with oracle.flush_denormals(flush):
            y = oracle.chain_process(procs, T, co, st, None, freq, n_threads=4)
        for a in (co, st0, y, st):
            a.setflags(write=False)
        _cache[key] = (co, st0, y, st)
    return _cache[key]


@pytest.fixture(scope="module")
def eng():
    import madronalib_amd as ml
    e = ml.Engine(0)
    e.mixdown_reserve(V, T)
    yield e
    e.set_flush_denormals(False)
    e.close()


def make_bank(eng, procs, co, st0):
    bank = eng.bank(procs, V)
    assert bank.fused and bank.kernel_name.startswith("chain_kernel<mldev::Chain<2")
    bank.set_all_coeffs(co)
    bank.set_all_state(st0.copy())
    bank.set_input_const(voices()[0])
    return bank


@pytest.mark.parametrize("layout", [pytest.param(Layout.QUAD, id="quad"), pytest.param(Layout.ROWS, id="rows")])
@pytest.mark.parametrize("procs", CHAINS)
def test_process_in_one_launch(eng, oracle, procs, layout):
    co, st0, y, st = reference(oracle, procs)
    (got,), gst, fused = _run_gpu(eng, procs, V, T, co, st0.copy(), None, voices()[0], layout)
    assert fused
    assert_bits_equal(got, y, True, "output")
    assert_bits_equal(gst, st, False, "final state")


@pytest.mark.parametrize("procs", CHAINS)
def test_launches_of_one_and_two_vectors_give_the_single_launch(eng, oracle, procs):
    co, st0, y, st = reference(oracle, procs)
    bank = make_bank(eng, procs, co, st0)
    got = np.concatenate([bank.process_host(1, None, Layout.QUAD), bank.process_host(2, None, Layout.QUAD)], 1)
    gst = bank.get_all_state()
    bank.close()
    assert_bits_equal(got, y, True, "launches of 1 + 2 against the oracle's single run")
    assert_bits_equal(gst, st, False, "final state")


@pytest.mark.parametrize("with_gains,flush", [pytest.param(False, False, id="plain"), pytest.param(True, False, id="gains"),
                                              pytest.param(True, True, id="gains-flush")])
def test_process_mixdown(eng, oracle, with_gains, flush):
    """The mix form (V is no multiple of 64: the last wavefront's spare lanes, i.e. the SCALED loop there and the plain one elsewhere),
    with and without gains; with gains also with denormal flushing on."""
    co, st0, y, st = reference(oracle, SAW_BP_GAIN, flush)
    gains = special_gains(V) if with_gains else None
    with oracle.flush_denormals(flush):
        want = oracle.mixdown(y, gains)
    eng.set_flush_denormals(flush)
    try:
        bank = make_bank(eng, SAW_BP_GAIN, co, st0)
        d_out = eng.alloc(4 * 64 * T)
        bank.process_mixdown(T, d_out, None, Layout.QUAD, None if gains is None else eng.to_device(gains))
        got, gst = d_out.download(np.float32, 64 * T), bank.get_all_state()
        bank.close()
    finally:
        eng.set_flush_denormals(False)
    assert np.isfinite(want).all() and np.abs(want).max() > 1e-6
    assert_bits_equal(got, want, True, f"mixdown gains={with_gains} flush={flush}")
    assert_bits_equal(gst, st, False, "final state")


def listed_reference(oracle, procs):
    co, st0, y, st = reference(oracle, procs)
    L = LIST.astype(np.int64)
    after = st0.copy()
    after[:, L] = st[:, L]           # (voices are independent: the listed ones end where the full run leaves them, the others stay)
    return co, st0, y[L], after


@pytest.mark.parametrize("procs", CHAINS)
def test_process_listed_with_peaks(eng, oracle, procs):
    co, st0, yl, after = listed_reference(oracle, procs)
    K = LIST.size
    bank = make_bank(eng, procs, co, st0)
    bank.set_voice_list(LIST)
    d_out, d_peak, d_vm = eng.alloc(4 * K * 64 * T), eng.alloc(4 * K), eng.alloc(4 * K * 64 * T)
    bank.process_listed(T, d_out, Layout.QUAD, d_peak=d_peak)
    eng.layout_convert(d_out, Layout.QUAD, d_vm, Layout.VOICE_MAJOR, K, T)
    got, peaks, gst = d_vm.download(np.float32, K * 64 * T).reshape(K, 64 * T), d_peak.download(np.uint32), bank.get_all_state()
    bank.close()
    assert_bits_equal(got, yl, True, "listed output")
    assert np.isfinite(yl).all()       # (a zero, negative, infinite or NaN frequency does not reach a SawGen's output)
    assert_bits_equal(peaks, expected_peaks(yl), False, "peaks")
    assert_bits_equal(gst, after, False, "state: the listed voices advanced, the others where they were")


@pytest.mark.parametrize("with_gains", [pytest.param(False, id="plain"), pytest.param(True, id="gains")])
def test_process_listed_mixdown_with_peaks(eng, oracle, with_gains):
    co, st0, yl, after = listed_reference(oracle, SAW_BP_GAIN)
    K = LIST.size
    gains = special_gains(V) if with_gains else None
    want = oracle.mixdown(yl, None if gains is None else np.ascontiguousarray(gains[LIST.astype(np.int64)]))
    bank = make_bank(eng, SAW_BP_GAIN, co, st0)
    bank.set_voice_list(LIST)
    d_out, d_peak = eng.alloc(4 * 64 * T), eng.alloc(4 * K)
    bank.process_listed_mixdown(T, d_out, None, Layout.QUAD, None if gains is None else eng.to_device(gains), d_peak)
    got, peaks, gst = d_out.download(np.float32, 64 * T), d_peak.download(np.uint32), bank.get_all_state()
    bank.close()
    assert np.isfinite(want).all() and np.abs(want).max() > 1e-6
    assert_bits_equal(got, want, True, f"listed mixdown gains={with_gains}")
    assert_bits_equal(peaks, expected_peaks(yl), False, "peaks (before the gain)")
    assert_bits_equal(gst, after, False, "state")
