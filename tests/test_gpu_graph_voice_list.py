"""Voice lists for graphs on the device: mlgpu_graph_set_voice_list and mlgpu_graph_process_listed (the listed form of the generated
kernel) - a listed call behaves as a graph of K voices made of voices L[0] ... L[K-1], and nobody else is touched.

Expected values (graph_voice_list_cases). Graphs without rings: graph_oracle.evaluate on the K gathered voices, the state taken from
and scattered back into the full graph's state, oracle.mixdown of the K rows, the peaks in numpy. Graphs with rings (ring memory
cannot be read back): a plain K-voice graph of the same description on the same device, run from clear with the gathered tables and
inputs - the existing graph tests pin that one to the oracle. All comparisons are bit-exact.

Every graph object is made anew per test; the kernels are compiled once per process (identical sources share a module)."""
import types

import numpy as np
import pytest

import graph_voice_list_cases as cases
from graph_voice_list_cases import LISTS, T, V, build_graph, expected_listed, expected_mixdown, expected_peaks, gathered, load_tables
from inputs import assert_bits_equal, lcg_noise
from madronalib_amd.constants import Layout, Status

GUARD = np.uint32(0x7FC5A5A5)   # what the memory around an output holds before a launch
ALL_LISTS = ("last", "wave", "k80", "k2100", "all", "empty")
_synth = {}


@pytest.fixture(scope="module")
def eng():
    import madronalib_amd as ml
    e = ml.Engine(0)
    yield e
    e.set_flush_denormals(False)
    e.close()


def synth(oracle, tiny=False):
    if tiny not in _synth:
        _synth[tiny] = cases.synth_case(oracle, tiny)
    return _synth[tiny]


def to_layout(eng, rows, layout, vectors):
    """[R][64 vectors] numpy -> a device signal of R rows in `layout`."""
    rows = np.ascontiguousarray(rows, np.float32)
    d = eng.to_device(rows)
    if layout in (Layout.VOICE_MAJOR, Layout.BROADCAST):
        return d
    d2 = eng.alloc(rows.nbytes)
    eng.layout_convert(d, Layout.VOICE_MAJOR, d2, layout, rows.shape[0], vectors)
    return d2


def guarded(eng, words, guard_words):
    d = eng.alloc(4 * (words + guard_words))
    d.upload(np.full(words + guard_words, GUARD, np.uint32))
    return d


def signals(eng, case, t0, n, in_layout):
    """The launch's device inputs and controls for DSPVectors [t0, t0 + n)."""
    d_in = [to_layout(eng, a[:, 64 * t0:64 * (t0 + n)], in_layout, n) for a in case.inputs.values()]
    d_ctl = [eng.to_device(np.ascontiguousarray(a[:, t0:t0 + n].T)) for a in case.controls.values()]
    return d_in, d_ctl


def run_listed(eng, g, case, K, splits, in_layout=Layout.QUAD, out_layout=Layout.QUAD, with_peaks=True):
    """process_listed over launches of `splits` DSPVectors with the list the graph has. Every output has one guard row behind it, d_peak[K]
    one guard word, that must come back untouched. Returns (the outputs: [K][64 T], or [64 T] for a mixed-down one; each launch's peaks)."""
    outs, peaks, t0 = [[] for _ in case.outputs], [], 0
    for n in splits:
        d_in, d_ctl = signals(eng, case, t0, n, in_layout)
        rows = [1 if o in case.mix else K for o in range(len(case.outputs))]
        d_out = [guarded(eng, r * 64 * n, 64 * n) for r in rows]
        d_peak = guarded(eng, K, 1) if with_peaks else None
        g.process_listed(n, d_in, d_out, in_layout, out_layout, d_ctl, d_peak)
        for o, (d, r) in enumerate(zip(d_out, rows)):
            raw = d.download(np.uint32)
            assert (raw[r * 64 * n:] == GUARD).all(), "the row behind the output was written"
            if o in case.mix or K == 0:
                outs[o].append(raw[:r * 64 * n].view(np.float32).reshape(r, 64 * n))
            else:
                d_vm = eng.alloc(4 * K * 64 * n)
                eng.layout_convert(d, out_layout, d_vm, Layout.VOICE_MAJOR, K, n)
                outs[o].append(d_vm.download(np.float32, K * 64 * n).reshape(K, 64 * n))
        if with_peaks:
            pk = d_peak.download(np.uint32)
            assert pk[K] == GUARD, "the word behind d_peak[K] was written"
            peaks.append(pk[:K].copy())
        t0 += n
    outs = [np.concatenate(o, 1) for o in outs]
    return [o[0] if i in case.mix else o for i, o in enumerate(outs)], peaks


def run_plain(eng, g, case, n_voices, n=T):
    """mlgpu_graph_process of all the graph's voices: the outputs [n_voices][64 n] ([64 n] for a mixed-down one)."""
    d_in, d_ctl = signals(eng, case, 0, n, Layout.VOICE_MAJOR)
    d_out = [eng.alloc(4 * (1 if o in case.mix else n_voices) * 64 * n) for o in range(len(case.outputs))]
    g.process(n, d_in, d_out, Layout.VOICE_MAJOR, Layout.VOICE_MAJOR, d_ctl)
    return [d.download(np.float32) if o in case.mix else d.download(np.float32).reshape(n_voices, 64 * n) for o, d in enumerate(d_out)]


def state_nodes(case):
    return [n["name"] for n in case.desc if n["type"] in ("proc", "feedback")]


def read_tables(g, case):
    """Every state, param and coefficient row of the graph: {key: [rows][V] uint32}."""
    t = {}
    for name in state_nodes(case):
        t[("state", name)] = np.stack([g.get_state(name, i) for i in range(g.num_state(name))])
    for name in case.params:
        t[("param", name)] = g.get_param(name).view(np.uint32)[None, :].copy()
    for name, co in case.coeffs.items():
        t[("coeff", name)] = np.stack([g.get_coeff(name, i).view(np.uint32) for i in range(co.shape[0])])
    return t


def check_peaks(peaks, ys, splits, what):
    """The peaks of each launch are those of that launch's samples alone (written once per launch, not accumulated)."""
    t0 = 0
    for pk, n in zip(peaks, splits):
        assert_bits_equal(pk, expected_peaks([y[:, 64 * t0:64 * (t0 + n)] for y in ys]), False, f"{what}: peaks of the launch of DSPVectors {t0}..{t0 + n - 1}")
        t0 += n


def check_synth(eng, oracle, lname, flush=False, in_layout=Layout.QUAD, out_layout=Layout.QUAD, tiny=False, case=None):
    case = case or synth(oracle, tiny)
    L = LISTS[lname]
    K, rest = L.size, np.setdiff1d(np.arange(V), L)
    what = f"synth list={lname} K={K} flush={flush} in={int(in_layout)} out={int(out_layout)}"
    states = {k: a.copy() for k, a in case.states.items()}
    ys = expected_listed(oracle, case, L, states, 0, T, flush)
    mix = expected_mixdown(oracle, ys[1], flush)
    eng.set_flush_denormals(flush)
    try:
        g = build_graph(eng, case)
        g.reserve_mixdown(T)
        load_tables(g, case)
        g.set_voice_list(L)
        assert g.voice_list_size == K
        before = read_tables(g, case)
        one, peaks_one = run_listed(eng, g, case, K, [T], in_layout, out_layout)
        after = read_tables(g, case)
        load_tables(g, case)
        split, peaks_split = run_listed(eng, g, case, K, [1, T - 1], in_layout, out_layout)
        after_split = read_tables(g, case)
        g.close()
    finally:
        eng.set_flush_denormals(False)
    if K:
        assert np.isfinite(ys[0]).all() and np.abs(ys[0]).max() > 1e-3 and (tiny or np.abs(ys[1]).max() > 1e-3), what
    else:
        assert (one[1].view(np.uint32) == 0).all(), what + ": the mixdown of no voices is +0.0"
    assert_bits_equal(one[0], ys[0], True, what + ": the plain output against the oracle")
    assert_bits_equal(one[1], mix, True, what + ": the mixed-down output against the oracle's voices and tree")
    for o in range(2):
        assert_bits_equal(split[o], one[o], True, what + f": output {o}, launches of 1 + 2 against one launch")
    check_peaks(peaks_one, ys, [T], what)
    check_peaks(peaks_split, ys, [1, T - 1], what + " (1 + 2)")
    for key in before:
        if key[0] == "state":
            assert_bits_equal(after[key][:, L], states[key[1]][:, L], False, what + f": {key} of the listed voices against the oracle")
            assert_bits_equal(after[key][:, rest], before[key][:, rest], False, what + f": {key} of the unlisted voices against the download before the call")
        else:
            assert_bits_equal(after[key], before[key], False, what + f": {key} against the download before the call")
        assert_bits_equal(after_split[key], after[key], False, what + f": {key} after 1 + 2 against one launch")
    return one, ys


@pytest.mark.gpu
@pytest.mark.parametrize("lname", ALL_LISTS)
def test_synth_voice_listed(eng, oracle, lname):
    """The synth voice (SawGen and PulseGen on one per-voice frequency, an input, a Lopass, a control; a plain and a mixed-down
    output), V = 2352, per-voice phases and filter memories. One launch of 3 DSPVectors and launches of 1 + 2: outputs, guard rows,
    the K-voice mixdown tree, peaks, the listed voices' state against the oracle, every state, param and coefficient word of the
    unlisted voices against a download taken before the call."""
    unequal, odd, dense = cases.irregular_voices()
    L = LISTS["k80"]
    for wave in (L[:64], L[64:]):   # both wavefronts of k80 hold the three kinds of voice
        assert np.intersect1d(wave, unequal).size and np.intersect1d(wave, odd).size and np.setdiff1d(wave, np.concatenate([unequal, odd, dense])).size > 8
    check_synth(eng, oracle, lname)


@pytest.mark.gpu
@pytest.mark.parametrize("flush", [pytest.param(False, id="ieee"), pytest.param(True, id="flush")])
@pytest.mark.parametrize("lname", ["k80", "k2100"])
def test_synth_voice_in_both_float_modes(eng, oracle, lname, flush):
    """The control in the 1e-39 range: every sample of the second output is denormal (ieee) or flushed to zero (flush), and its
    mixdown adds them up; the peaks are integer maxima of the stored bits in both modes."""
    _, ys = check_synth(eng, oracle, lname, flush=flush, tiny=True)
    mags = np.abs(ys[1])
    assert (mags == 0).all() if flush else ((mags > 0) & (mags < np.float32(1.17549435e-38))).mean() > 0.9


@pytest.mark.gpu
@pytest.mark.parametrize("in_layout,out_layout", [(Layout.VOICE_MAJOR, Layout.VOICE_MAJOR), (Layout.QUAD, Layout.VOICE_MAJOR), (Layout.VOICE_MAJOR, Layout.QUAD)])
def test_input_and_output_layouts(eng, oracle, in_layout, out_layout):
    check_synth(eng, oracle, "k80", in_layout=in_layout, out_layout=out_layout)


@pytest.mark.gpu
def test_a_broadcast_input_and_an_input_group(eng, oracle):
    """MLGPU_LAYOUT_BROADCAST set for the input (mlgpu_graph_set_input_layout): the one row for every voice. An input of V / 16 rows
    (mlgpu_graph_set_input_group): the voice at list position i reads row L[i] / 16."""
    base = synth(oracle)
    row = np.ascontiguousarray(base.inputs["x"][3:4])
    as_rows = types.SimpleNamespace(**{**vars(base), "inputs": {"x": np.ascontiguousarray(np.repeat(row, V, axis=0))}})
    want, _ = check_synth(eng, oracle, "k80", case=as_rows, in_layout=Layout.VOICE_MAJOR)
    L = LISTS["k80"]
    g = build_graph(eng, base)
    g.reserve_mixdown(T)
    g.set_input_layout(0, Layout.BROADCAST)
    load_tables(g, base)
    g.set_voice_list(L)
    one_row = types.SimpleNamespace(**{**vars(base), "inputs": {"x": row}})
    got, _ = run_listed(eng, g, one_row, L.size, [T], Layout.VOICE_MAJOR, Layout.QUAD)
    g.close()
    for o in range(2):
        assert_bits_equal(got[o], want[o], True, f"output {o}: a broadcast input against the same row per voice")
    grouped = types.SimpleNamespace(**{**vars(base), "inputs": {"x": np.ascontiguousarray(base.inputs["x"][:V // 16])}, "groups": {"x": 16}})
    check_synth(eng, oracle, "k80", case=grouped)
    check_synth(eng, oracle, "k2100", case=grouped, in_layout=Layout.VOICE_MAJOR)


# ---- graphs with rings: against a plain K-voice graph ---------------------------------------------------------------------------------
def k_voice_reference(eng, case, L, n=T):
    """A plain graph of the K voices L with the same description, from clear: (outputs, its tables)."""
    k = gathered(case, L)
    gk = build_graph(eng, k, L.size, voice_lists=False)
    load_tables(gk, k)
    outs = run_plain(eng, gk, k, L.size, n)
    tables = read_tables(gk, k)
    gk.close()
    return outs, tables


def check_rings(eng, case, lname, what):
    L = LISTS[lname]
    C = np.setdiff1d(np.arange(V), L).astype(np.uint32)
    g = build_graph(eng, case)
    assert g.delay_layout == 0
    load_tables(g, case)
    g.set_voice_list(L)
    before = read_tables(g, case)
    got, peaks = run_listed(eng, g, case, L.size, [1, T - 1])      # (launches of 1 + 2 against the K-voice graph's one launch)
    after = read_tables(g, case)
    want, want_tables = k_voice_reference(eng, case, L)
    for o in range(len(case.outputs)):
        assert np.abs(want[o]).max() > 1e-3
        assert_bits_equal(got[o], want[o], True, f"{what} list={lname}: output {o} against a {L.size}-voice graph")
    check_peaks(peaks, want, [1, T - 1], f"{what} list={lname}")
    for key in before:
        assert_bits_equal(after[key][:, L], want_tables[key], False, f"{what} list={lname}: {key} of the listed voices against the {L.size}-voice graph")
        assert_bits_equal(after[key][:, C], before[key][:, C], False, f"{what} list={lname}: {key} of the unlisted voices against the download before the call")
    if C.size:
        # the complement, on the same graph: its rings were not touched and no time has passed for it - a C-voice graph from clear
        g.set_voice_list(C)
        got_c, _ = run_listed(eng, g, case, C.size, [T])
        want_c, tables_c = k_voice_reference(eng, case, C)
        for o in range(len(case.outputs)):
            assert_bits_equal(got_c[o], want_c[o], True, f"{what} list={lname}: output {o} of the complement against a {C.size}-voice graph from clear")
        final = read_tables(g, case)
        for key in before:
            assert_bits_equal(final[key][:, C], tables_c[key], False, f"{what} list={lname}: {key} of the complement")
            assert_bits_equal(final[key][:, L], after[key][:, L], False, f"{what} list={lname}: {key} of the first list after the complement ran")
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lname", ["k80", "k2100", "all"])
def test_string_graph_listed(eng, lname):
    """input -> FractionalDelay (per-voice delay time) -> OnePole -> gain -> back in through a feedback node; ring layout 0, one ring."""
    check_rings(eng, cases.ring_case("string"), lname, "string")


@pytest.mark.gpu
@pytest.mark.parametrize("lname", ["k80", "all"])
def test_three_ring_graph_listed(eng, lname):
    """Three rings: the layout-0 ring reads are issued early by LDS-DMA, into landing slots that go by lane while the rows go by voice."""
    case = cases.ring_case("three")
    g = build_graph(eng, case)
    assert "ldsEarly" in g.listed_source()
    g.close()
    check_rings(eng, case, lname, "three rings")


@pytest.mark.gpu
def test_upsample_region_graph_listed(eng):
    """fn = Lopass at twice the rate inside an UPSAMPLE_2X region (its HalfBandFilters' state per voice), then a Gain: k80 against an
    80-voice graph, the unlisted voices' state untouched."""
    import madronalib_amd as ml
    L = LISTS["k80"]
    Li = L.astype(np.int64)
    rng = np.random.default_rng(31)
    lp = np.stack([ml.Lopass.makeCoeffs(float(om), 0.9) for om in rng.uniform(0.02, 0.2, 8)], 1)[:, rng.integers(0, 8, V)].astype(np.float32)
    gain = rng.uniform(0.2, 1.0, V).astype(np.float32)
    x = lcg_noise(np.arange(V, dtype=np.uint32) + 9, 64 * T)

    def make(n, idx, voice_lists):
        g = cases.upsample_graph(eng, n, voice_lists)
        g.compile()
        g.clear()
        for i in range(3):
            g.set_coeff("rlp", i, np.ascontiguousarray(lp[i, idx]))
        g.set_coeff("gain", 0, np.ascontiguousarray(gain[idx]))
        return g
    full, small = make(V, np.arange(V), True), make(L.size, Li, False)
    n_nodes = full.L.mlgpu_graph_num_nodes(full.h)
    state_of = lambda g: [np.stack([g.get_state(i, w) for w in range(g.num_state(i))]) for i in range(n_nodes) if g.num_state(i) > 0]  # noqa: E731
    before = state_of(full)
    full.set_voice_list(L)
    d_out, d_peak = eng.alloc(4 * L.size * 64 * T), eng.alloc(4 * L.size)
    full.process_listed(T, [eng.to_device(x)], [d_out], Layout.VOICE_MAJOR, Layout.VOICE_MAJOR, d_peak=d_peak)
    d_want = eng.alloc(4 * L.size * 64 * T)
    small.process(T, [eng.to_device(np.ascontiguousarray(x[Li]))], [d_want], Layout.VOICE_MAJOR, Layout.VOICE_MAJOR)
    got, want = d_out.download(np.float32).reshape(L.size, 64 * T), d_want.download(np.float32).reshape(L.size, 64 * T)
    after, small_state = state_of(full), state_of(small)
    full.close(), small.close()
    assert np.abs(want).max() > 1e-3
    assert_bits_equal(got, want, True, "the region graph's output against an 80-voice graph")
    assert_bits_equal(d_peak.download(np.uint32), expected_peaks([want]), False, "peaks")
    rest = np.setdiff1d(np.arange(V), Li)
    assert len(before) == 3      # (the two HalfBandFilters of the region and the Lopass inside it)
    for b, a, s in zip(before, after, small_state):
        assert_bits_equal(a[:, Li], s, False, "state of the listed voices against the 80-voice graph")
        assert_bits_equal(a[:, rest], b[:, rest], False, "state of the unlisted voices")


# ---- peaks ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_peaks_show_a_nan_and_a_silent_voice(eng, oracle):
    """A Gain on a streamed input: the voice whose gain coefficient is 0 reports 0, the voice whose coefficient is a NaN a value above
    0x7f800000 (held to the threshold: NaN payloads are not portable), every other voice the numpy value; d_peak = NULL is accepted."""
    desc, outputs = cases.gain_desc()
    L = LISTS["k80"]
    Li = L.astype(np.int64)
    nan_pos, silent_pos = 3, 70      # list positions: in the first wavefront and in the last, partial one
    rng = np.random.default_rng(5)
    gain = rng.uniform(0.1, 1.0, (1, V)).astype(np.float32)
    gain[0, Li[nan_pos]], gain[0, Li[silent_pos]] = np.float32(np.nan), np.float32(0.0)
    case = types.SimpleNamespace(desc=desc, outputs=outputs, mix=(), inputs={"x": lcg_noise(np.arange(V, dtype=np.uint32) + 1, 64 * T)}, groups={},
                                 controls={}, params={}, coeffs={"gain": gain}, states={"gain": oracle.chain_default_state([desc[1]["kind"]], V)})
    g = build_graph(eng, case)
    load_tables(g, case)
    g.set_voice_list(L)
    (got,), peaks = run_listed(eng, g, case, L.size, [T])
    load_tables(g, case)
    (again,), none = run_listed(eng, g, case, L.size, [T], with_peaks=False)
    g.close()
    (y,) = expected_listed(oracle, case, L, {k: a.copy() for k, a in case.states.items()})
    want = expected_peaks([y])
    finite = np.arange(L.size) != nan_pos
    assert want[silent_pos] == 0 and (want[finite] < 0x7F800000).all() and (want[finite & (np.arange(L.size) != silent_pos)] > 0).all()
    assert_bits_equal(got, y, True, "Gain with a NaN and a zero coefficient")
    assert_bits_equal(again, got, True, "the same launch without peaks")
    assert none == []
    assert_bits_equal(peaks[0][finite], want[finite], False, "peaks against numpy")
    assert peaks[0][silent_pos] == 0
    assert peaks[0][nan_pos] > 0x7F800000, f"the NaN voice reports 0x{int(peaks[0][nan_pos]):08x}"


# ---- stream order, sequences, process next to listed --------------------------------------------------------------------------------------
def refused(status, words, fn, *args, **kw):
    import madronalib_amd as ml
    with pytest.raises(ml.MlgpuError) as ei:
        fn(*args, **kw)
    assert ei.value.status == status, str(ei.value)
    assert all(w in str(ei.value) for w in words), str(ei.value)


@pytest.mark.gpu
def test_updates_lists_and_process_calls_are_ordered_on_the_stream(eng):
    """The string graph, after two DSPVectors of list A: apply_updates (CLEAR_RINGS of a voice of B, a PARAM of another), set_voice_list(B),
    process_listed, set_voice_list(C), process_listed - issued back to back, nothing waited for, against the same steps with an
    engine sync between each. Then lists that are refused (descending, out of range, longer than the reserve): the list in force
    stays, and the next launch is C's."""
    import madronalib_amd as ml
    case = cases.ring_case("string")
    rng = np.random.default_rng(17)
    A = np.sort(rng.choice(V, 300, replace=False)).astype(np.uint32)
    B = np.sort(np.concatenate([A[::3], np.setdiff1d(np.arange(V), A)[5:400:7]])).astype(np.uint32)
    C = np.unique(np.concatenate([A[1::2], B[::2], np.arange(2300, V)])).astype(np.uint32)
    stolen, retuned = int(A[::3][5]), int(A[::3][50])     # (voices of A and of B)
    assert len({A.size, B.size, C.size}) == 3
    results = []
    for synced in (False, True):
        g = build_graph(eng, case)
        load_tables(g, case)
        g.reserve_voice_list(max(A.size, B.size, C.size))
        g.reserve_updates(4096)
        updates = [ml.Update.clear_rings(-1, stolen, 1), ml.Update.param(g.ids["dt"], retuned, 1, 33.25)]
        d_x = [eng.to_device(np.ascontiguousarray(case.inputs["x"][:, 64 * t:64 * (t + 1)])) for t in range(T)]
        d_outs = [eng.alloc(4 * l.size * 64) for l in (A, A, B, C, C)]
        d_peak = eng.alloc(4 * V)
        wait = eng.sync if synced else (lambda: None)
        eng.sync()
        g.set_voice_list(A), wait()
        g.process_listed(1, [d_x[0]], [d_outs[0]], Layout.VOICE_MAJOR, Layout.VOICE_MAJOR), wait()
        g.process_listed(1, [d_x[1]], [d_outs[1]], Layout.VOICE_MAJOR, Layout.VOICE_MAJOR), wait()
        g.apply_updates(updates), wait()
        g.set_voice_list(B), wait()
        g.process_listed(1, [d_x[2]], [d_outs[2]], Layout.VOICE_MAJOR, Layout.VOICE_MAJOR, d_peak=d_peak), wait()
        g.set_voice_list(C), wait()
        g.process_listed(1, [d_x[0]], [d_outs[3]], Layout.VOICE_MAJOR, Layout.VOICE_MAJOR), wait()
        if not synced:
            refused(Status.ERR_INVALID, ["graph_set_voice_list", "ascending", "position 1"], g.set_voice_list, [40, 9])
            refused(Status.ERR_RANGE, ["graph_set_voice_list", "position 3", str(V)], g.set_voice_list, [0, 1, 2, V])
            refused(Status.ERR_RANGE, ["graph_set_voice_list", "reserved"], g.set_voice_list, np.arange(A.size + 1))
            assert g.voice_list_size == C.size
        g.process_listed(1, [d_x[1]], [d_outs[4]], Layout.VOICE_MAJOR, Layout.VOICE_MAJOR), wait()
        results.append(([d.download(np.float32) for d in d_outs], d_peak.download(np.uint32)[:B.size], read_tables(g, case)))
        g.close()
    (outs, peaks, tables), (outs_s, peaks_s, tables_s) = results
    for k, name in enumerate(("A", "A again", "B after the updates", "C", "C after the refused lists")):
        assert np.abs(outs_s[k]).max() > 1e-3
        assert_bits_equal(outs[k], outs_s[k], True, f"the block of list {name}: back to back against synced")
    assert_bits_equal(peaks, peaks_s, False, "peaks of B")
    for key in tables:
        assert_bits_equal(tables[key], tables_s[key], False, f"{key} at the end")
    # the updates arrived: the param row holds the new delay time, the stolen voice's feedback vector started again from zeros
    assert tables_s[("param", "dt")][0, retuned] == np.float32(33.25).view(np.uint32)


@pytest.mark.gpu
def test_recorded_into_a_sequence(eng, oracle):
    """set_voice_list is refused while recording; a recorded process_listed reads whichever list is on the device when it is replayed:
    after the contents change at equal length the replay gives what a direct call with the new list gives."""
    case = synth(oracle)
    A = LISTS["k80"]
    A2 = np.sort(np.random.default_rng(23).choice(V, A.size, replace=False)).astype(np.uint32)
    assert (A2 != A).any()
    graphs = [build_graph(eng, case), build_graph(eng, case)]
    for g in graphs:
        g.reserve_mixdown(1)
        load_tables(g, case)
    d_in, d_ctl = signals(eng, case, 0, 1, Layout.QUAD)
    d_out, d_peak = [eng.alloc(4 * A.size * 64), eng.alloc(4 * 64)], eng.alloc(4 * A.size)
    take = lambda: (d_out[0].download(np.float32), d_out[1].download(np.float32), d_peak.download(np.uint32))  # noqa: E731
    direct, replayed = [], []
    for l in (A, A2):
        graphs[0].set_voice_list(l)
        graphs[0].process_listed(1, d_in, d_out, Layout.QUAD, Layout.QUAD, d_ctl, d_peak)
        direct.append(take())
    graphs[1].reserve_voice_list(A.size)
    graphs[1].set_voice_list(A)
    with eng.record() as seq:
        refused(Status.ERR_INVALID, ["graph_set_voice_list", "recording"], graphs[1].set_voice_list, A2)
        graphs[1].process_listed(1, d_in, d_out, Layout.QUAD, Layout.QUAD, d_ctl, d_peak)
    assert seq.num_nodes >= 2
    seq.launch()
    replayed.append(take())
    graphs[1].set_voice_list(A2)
    seq.launch()
    replayed.append(take())
    for k in range(2):
        assert_bits_equal(replayed[k][0], direct[k][0], True, f"replay {k}: the plain output")
        assert_bits_equal(replayed[k][1], direct[k][1], True, f"replay {k}: the mixed-down output")
        assert_bits_equal(replayed[k][2], direct[k][2], False, f"replay {k}: peaks")
    assert (direct[0][0].view(np.uint32) != direct[1][0].view(np.uint32)).any()
    ta, tb = read_tables(graphs[0], case), read_tables(graphs[1], case)
    for key in ta:
        assert_bits_equal(tb[key], ta[key], False, f"{key} after two replays")
    for g in graphs:
        g.close()


@pytest.mark.gpu
def test_process_next_to_listed_calls(eng, oracle):
    """A plain launch of all voices after a listed launch sees exactly the state the listed launch left (the oracle: the listed voices
    one launch ahead of the others). And mlgpu_graph_process of a graph with voice lists enabled gives the bits of the same graph
    without."""
    case = synth(oracle)
    L = LISTS["k80"]
    states = {k: a.copy() for k, a in case.states.items()}
    expected_listed(oracle, case, L, states)
    ys = expected_listed(oracle, case, np.arange(V), states)
    want = [ys[0], expected_mixdown(oracle, ys[1])]
    g = build_graph(eng, case)
    g.reserve_mixdown(T)
    load_tables(g, case)
    g.set_voice_list(L)
    run_listed(eng, g, case, L.size, [T])
    got = run_plain(eng, g, case, V)
    tables = read_tables(g, case)
    load_tables(g, case)
    with_lists = run_plain(eng, g, case, V)
    assert g.tuning()[1:] == (1, 1)
    g.close()
    for o in range(2):
        assert_bits_equal(got[o], want[o], True, f"output {o} of process after process_listed against the oracle")
    for name in case.states:
        assert_bits_equal(tables[("state", name)], states[name], False, f"state of {name}")
    off = build_graph(eng, case, voice_lists=False)
    off.reserve_mixdown(T)
    load_tables(off, case)
    without = run_plain(eng, off, case, V)
    refused(Status.ERR_INVALID, ["graph_process_listed", "mlgpu_graph_enable_voice_lists"], off.process_listed, T, [0], [0, 0], d_controls=[0])
    off.close()
    for o in range(2):
        assert_bits_equal(with_lists[o], without[o], True, f"output {o}: process with voice lists enabled against without")


@pytest.mark.gpu
def test_compile_async_loads_both_kernels(eng, oracle):
    """mlgpu_graph_compile_async / _poll on a graph with voice lists: once the poll says ready, the listed kernel is loaded too - a
    listed launch follows at once and gives the oracle's bits."""
    import time
    case = synth(oracle)
    L = LISTS["k80"]
    g = build_graph(eng, case, compile_now=False)
    g.compile_async()
    while not g.compile_poll():
        time.sleep(0.001)
    g.reserve_mixdown(T)
    load_tables(g, case)
    g.set_voice_list(L)
    got, peaks = run_listed(eng, g, case, L.size, [T])
    g.close()
    ys = expected_listed(oracle, case, L, {k: a.copy() for k, a in case.states.items()})
    assert_bits_equal(got[0], ys[0], True, "the plain output against the oracle")
    assert_bits_equal(got[1], expected_mixdown(oracle, ys[1]), True, "the mixed-down output against the oracle")
    check_peaks(peaks, ys, [T], "after compile_async")
