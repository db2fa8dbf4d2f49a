"""A graph's listed group sums on the device: mlgpu_graph_reserve_voice_list_groups and mlgpu_graph_process_listed_groups (the
lane-plan form of the generated listed kernel) - the listed voices run as in mlgpu_graph_process_listed, every group-summed output
comes back as one row per listed instrument, the in-order float sum of that instrument's listed voices, and nobody else is touched.

Expected values (graph_voice_list_groups_cases). Graphs without rings: graph_oracle.evaluate on the K gathered voices, the state
taken from and scattered back into the full graph's state; the rows of a group-summed output accumulated per instrument from +0.0 with
the CPU checker's float32 add; the peaks in numpy. Graphs with rings: a plain K-voice graph of the same description on the same
device, its rows summed the same way. All comparisons are bit-exact.

Every graph object is made anew per test; the kernels are compiled once per process (identical sources share a module)."""
import types

import numpy as np
import pytest

import graph_voice_list_cases as base_cases
import graph_voice_list_groups_cases as cases
from graph_voice_list_groups_cases import (GROUPS, LISTS, T, V, build_group_graph, expected_listed, expected_outputs,
                                           expected_peaks, expected_plan, gathered, load_tables)
from inputs import assert_bits_equal
from madronalib_amd.constants import Layout, Status

GUARD = np.uint32(0x7FC5A5A5)   # what the memory around an output holds before a launch
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


def run_groups(eng, g, case, sums, K, J, splits, in_layout=Layout.QUAD, out_layout=Layout.QUAD, with_peaks=True):
    """process_listed_groups over launches of `splits` DSPVectors with the list the graph has. An output of `sums` has J rows, every
    other one K; each has one guard row behind it and d_peak[K] one guard word, which must come back untouched. Returns (the outputs,
    [rows][64 T]; each launch's peaks)."""
    outs, peaks, t0 = [[] for _ in case.outputs], [], 0
    rows = [J if o in sums else K for o in range(len(case.outputs))]
    for n in splits:
        d_in, d_ctl = signals(eng, case, t0, n, in_layout)
        d_out = [guarded(eng, r * 64 * n, 64 * n) for r in rows]
        d_peak = guarded(eng, K, 1) if with_peaks else None
        g.process_listed_groups(n, d_in, d_out, in_layout, out_layout, d_ctl, d_peak)
        for o, (d, r) in enumerate(zip(d_out, rows)):
            raw = d.download(np.uint32)
            assert (raw[r * 64 * n:] == GUARD).all(), f"the row behind output {o} was written"
            if r == 0:
                outs[o].append(np.zeros((0, 64 * n), np.float32))
                continue
            d_vm = eng.alloc(4 * r * 64 * n)
            eng.layout_convert(d, out_layout, d_vm, Layout.VOICE_MAJOR, r, n)
            outs[o].append(d_vm.download(np.float32, r * 64 * n).reshape(r, 64 * n))
        if with_peaks:
            pk = d_peak.download(np.uint32)
            assert pk[K] == GUARD, "the word behind d_peak[K] was written"
            peaks.append(pk[:K].copy())
        t0 += n
    return [np.concatenate(o, 1) for o in outs], peaks


def run_plain(eng, g, case, rows, n=T):
    """mlgpu_graph_process of all the graph's voices: the outputs, [rows[o]][64 n]."""
    d_in, d_ctl = signals(eng, case, 0, n, Layout.VOICE_MAJOR)
    d_out = [eng.alloc(4 * r * 64 * n) for r in rows]
    g.process(n, d_in, d_out, Layout.VOICE_MAJOR, Layout.VOICE_MAJOR, d_ctl)
    return [d.download(np.float32).reshape(r, 64 * n) for d, r in zip(d_out, rows)]


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
    """The peaks of each launch are those of that launch's samples alone, over every output, before the sums."""
    t0 = 0
    for pk, n in zip(peaks, splits):
        assert_bits_equal(pk, expected_peaks([y[:, 64 * t0:64 * (t0 + n)] for y in ys]), False, f"{what}: peaks of the launch of DSPVectors {t0}..{t0 + n - 1}")
        t0 += n


def check_plan(g, lname, G, what):
    N, pads, J, M = expected_plan(lname, G)
    assert g.voice_list_size == LISTS[lname].size, what
    got = g.listed_groups
    assert got.size == J and got.dtype == np.uint32 and (got == M).all(), what + ": the listed instruments"
    return J


def check_synth(eng, oracle, lname, G, summed=0, flush=False, in_layout=Layout.QUAD, out_layout=Layout.QUAD, tiny=False, case=None, split=False, tables=False):
    """The synth voice with output `summed` summed by G and the other one plain, against the oracle: one launch of T DSPVectors; with
    `split` also launches of 1 + 2; with `tables` every state, param and coefficient word before and after."""
    case = case or synth(oracle, tiny)
    L, sums = LISTS[lname], {summed: G}
    K, rest = L.size, np.setdiff1d(np.arange(V), L)
    what = f"synth list={lname} K={K} G={G} summed={summed} flush={flush} in={int(in_layout)} out={int(out_layout)}"
    states = {k: a.copy() for k, a in case.states.items()}
    ys = expected_listed(oracle, case, L, states, 0, T, flush)
    want = expected_outputs(oracle, ys, L, sums, flush)
    eng.set_flush_denormals(flush)
    try:
        g = build_group_graph(eng, case, sums)
        load_tables(g, case)
        g.reserve_voice_list_groups(max(K, 1))
        g.set_voice_list(L)
        J = check_plan(g, lname, G, what)
        before = read_tables(g, case) if tables else {}
        one, peaks_one = run_groups(eng, g, case, sums, K, J, [T], in_layout, out_layout)
        after = read_tables(g, case) if tables else {}
        if split:
            load_tables(g, case)
            two, peaks_two = run_groups(eng, g, case, sums, K, J, [1, T - 1], in_layout, out_layout)
            after_split = read_tables(g, case) if tables else {}
        g.close()
    finally:
        eng.set_flush_denormals(False)
    assert np.isfinite(ys[0]).all() and np.abs(ys[0]).max() > 1e-3 and (tiny or np.abs(ys[1]).max() > 1e-3), what
    assert want[summed].shape == (J, 64 * T) and want[1 - summed].shape == (K, 64 * T)
    assert_bits_equal(one[summed], want[summed], True, what + ": the rows of the listed instruments against the oracle")
    assert_bits_equal(one[1 - summed], want[1 - summed], True, what + ": the plain output against the oracle")
    check_peaks(peaks_one, ys, [T], what)
    if split:
        for o in range(2):
            assert_bits_equal(two[o], one[o], True, what + f": output {o}, launches of 1 + 2 against one launch")
        check_peaks(peaks_two, ys, [1, T - 1], what + " (1 + 2)")
    for key in before:
        if key[0] == "state":
            assert_bits_equal(after[key][:, L], states[key[1]][:, L], False, what + f": {key} of the listed voices against the oracle")
            assert_bits_equal(after[key][:, rest], before[key][:, rest], False, what + f": {key} of the unlisted voices against the download before the call")
        else:
            assert_bits_equal(after[key], before[key], False, what + f": {key} against the download before the call")
        if split:
            assert_bits_equal(after_split[key], after[key], False, what + f": {key} after 1 + 2 against one launch")
    return one, ys, want


SYNTH_CASES = [("k2100", G) for G in GROUPS] + [(lname, 16) for lname in ("straddle", "fit", "all", "last", "k80")]


@pytest.mark.gpu
@pytest.mark.parametrize("lname,G", SYNTH_CASES, ids=[f"{l}-{G}" for l, G in SYNTH_CASES])
def test_synth_voice_listed_groups(eng, oracle, lname, G):
    """The synth voice (SawGen and PulseGen on one per-voice frequency, an input, a Lopass, a control), output 0 summed by G, output 1
    plain, V = 2352, per-voice phases and filter memories: the rows of the listed instruments, the plain output's K rows, the guard
    rows, the peaks and the listed instruments against the oracle and the modelled plan. k80 carries the unequal, odd and dense
    voices next to regular ones."""
    if lname == "k80":
        unequal, odd, dense = base_cases.irregular_voices()
        lanes, _, pads, _ = cases.model_plan(LISTS["k80"], G)
        first = np.array([v for v in lanes[:64] if v != 0xFFFFFFFF])
        assert np.intersect1d(first, unequal).size and np.intersect1d(first, odd).size and np.intersect1d(first, dense).size
        assert np.setdiff1d(first, np.concatenate([unequal, odd, dense])).size > 8
    if lname == "straddle":
        assert expected_plan(lname, G)[1] == 2      # (the two pads sit in the MIDDLE of the launch: lanes 62 and 63)
    check_synth(eng, oracle, lname, G)


@pytest.mark.gpu
@pytest.mark.parametrize("flush", [pytest.param(False, id="ieee"), pytest.param(True, id="flush")])
def test_sums_through_the_denormal_range_in_both_float_modes(eng, oracle, flush):
    """The control in the 1e-39 range and output 1 - Lopass * control - the summed one: every term of a sum is denormal (ieee) or
    flushed to zero (flush), and so are the sums' steps."""
    _, ys, want = check_synth(eng, oracle, "k2100", 16, summed=1, flush=flush, tiny=True)
    mags = np.abs(ys[1])
    assert (mags == 0).all() if flush else ((mags > 0) & (mags < np.float32(1.17549435e-38))).mean() > 0.9
    assert (want[1] == 0).all() if flush else (np.abs(want[1]) > 0).mean() > 0.9


@pytest.mark.gpu
@pytest.mark.parametrize("G", [16, 4])
def test_every_voice_listed_gives_the_bits_of_process(eng, oracle, G):
    """The list of all voices: the group rows are those of mlgpu_graph_process of the same graph - its lane-shift sums (G = 4) and its
    16-voice strip (G = 16) - and the plain output is the same too."""
    case, L, sums = synth(oracle), LISTS["all"], {0: G}
    g = build_group_graph(eng, case, sums)
    load_tables(g, case)
    g.reserve_voice_list_groups(V)
    g.set_voice_list(L)
    assert check_plan(g, "all", G, f"all G={G}") == V // G
    got, _ = run_groups(eng, g, case, sums, V, V // G, [T])
    load_tables(g, case)
    want = run_plain(eng, g, case, [V // G, V])
    g.close()
    assert np.abs(want[0]).max() > 1e-3
    for o in range(2):
        assert_bits_equal(got[o], want[o], True, f"G={G}: output {o} of process_listed_groups with every voice listed against process")


@pytest.mark.gpu
@pytest.mark.parametrize("lname", ["k80", "straddle"])
def test_split_launches_and_the_unlisted_voices(eng, oracle, lname):
    """T = 3 as 1 + 2 gives the bits of one call; every state, param and coefficient word of the unlisted voices is what it was before
    the call, the listed voices' state words are the oracle's."""
    check_synth(eng, oracle, lname, 16, split=True, tables=True)


@pytest.mark.gpu
def test_a_lone_minus_zero_gives_plus_zero(eng, oracle):
    """A Gain on input rows of -0.0: the voice stores -0.0; alone in its instrument its row is (0 + -0.0) = +0.0 by bits."""
    case, L = cases.minus_zero_case(oracle)
    sums, G = {0: 4}, 4
    (y,) = expected_listed(oracle, case, L, {k: a.copy() for k, a in case.states.items()})
    (want,) = expected_outputs(oracle, [y], L, sums)
    M = np.unique(L.astype(np.int64) // G)
    lone = int(np.nonzero(M == 5 // G)[0][0])
    assert (y[list(L).index(5)].view(np.uint32) == 0x80000000).all() and (want[lone].view(np.uint32) == 0).all()
    g = build_group_graph(eng, case, sums)
    load_tables(g, case)
    g.reserve_voice_list_groups(L.size)
    g.set_voice_list(L)
    assert (g.listed_groups == M).all()
    (got,), peaks = run_groups(eng, g, case, sums, L.size, M.size, [T])
    g.close()
    assert (got[lone].view(np.uint32) == 0).all(), "the row of the lone -0.0 voice is not +0.0"
    assert_bits_equal(got, want, True, "Gain with -0.0 rows: the instruments' rows against the oracle")
    check_peaks(peaks, [y], [T], "Gain with -0.0 rows")
    assert peaks[0][list(L).index(5)] == 0


@pytest.mark.gpu
def test_an_input_group_of_the_instruments_size(eng, oracle):
    """P = G = 4: one input row per instrument, read by each of its listed voices."""
    base = synth(oracle)
    grouped = types.SimpleNamespace(**{**vars(base), "inputs": {"x": np.ascontiguousarray(base.inputs["x"][:V // 4])}, "groups": {"x": 4}})
    check_synth(eng, oracle, "k2100", 4, case=grouped)
    check_synth(eng, oracle, "k80", 4, case=grouped, in_layout=Layout.VOICE_MAJOR)


@pytest.mark.gpu
@pytest.mark.parametrize("out_layout", [Layout.QUAD, Layout.ROWS, Layout.VOICE_MAJOR], ids=["quad", "rows", "voice_major"])
def test_output_layouts(eng, oracle, out_layout):
    check_synth(eng, oracle, "k80", 16, in_layout=Layout.VOICE_MAJOR, out_layout=out_layout)


# ---- graphs with rings: against a plain K-voice graph whose rows are summed on the host ------------------------------------------------------
def k_voice_reference(eng, case, L, n=T):
    """A plain graph of the K voices L with the same description and no sums, from clear: (outputs [K][64 n], its tables)."""
    k = gathered(case, L)
    gk = build_group_graph(eng, k, {}, L.size, switch=False)
    load_tables(gk, k)
    outs = run_plain(eng, gk, k, [L.size] * len(case.outputs), n)
    tables = read_tables(gk, k)
    gk.close()
    return outs, tables


@pytest.mark.gpu
@pytest.mark.parametrize("lname", ["k80", "straddle"])
@pytest.mark.parametrize("which", ["string", "three"])
def test_ring_graphs_listed_groups(eng, oracle, which, lname):
    """The plucked string (one ring) and the three-ring graph (ring layout 0, the reads issued early by LDS-DMA into landing slots
    that go by lane), from clear, output 0 summed by 16: launches of 1 + 2 against a K-voice graph's one launch, its rows of output 0
    summed per instrument by the checker's float add; the unlisted voices' tables untouched."""
    case, L, sums = cases.ring_case(which), LISTS[lname], {0: 16}
    what = f"{which} list={lname}"
    rest = np.setdiff1d(np.arange(V), L)
    g = build_group_graph(eng, case, sums)
    assert g.delay_layout == 0 and ("ldsEarly" in g.listed_source()) == (which == "three")
    load_tables(g, case)
    g.reserve_voice_list_groups(L.size)
    g.set_voice_list(L)
    J = check_plan(g, lname, 16, what)
    before = read_tables(g, case)
    got, peaks = run_groups(eng, g, case, sums, L.size, J, [1, T - 1])
    after = read_tables(g, case)
    g.close()
    ys, want_tables = k_voice_reference(eng, case, L)
    want = expected_outputs(oracle, ys, L, sums)
    for o in range(len(case.outputs)):
        assert np.abs(want[o]).max() > 1e-3
        assert_bits_equal(got[o], want[o], True, f"{what}: output {o} against a {L.size}-voice graph" + (", summed per instrument" if o in sums else ""))
    check_peaks(peaks, ys, [1, T - 1], what)
    for key in before:
        assert_bits_equal(after[key][:, L], want_tables[key], False, f"{what}: {key} of the listed voices against the {L.size}-voice graph")
        assert_bits_equal(after[key][:, rest], before[key][:, rest], False, f"{what}: {key} of the unlisted voices against the download before the call")


# ---- refusals at run time -----------------------------------------------------------------------------------------------------------------
def refused(status, words, fn, *args, **kw):
    import madronalib_amd as ml
    with pytest.raises(ml.MlgpuError) as ei:
        fn(*args, **kw)
    assert ei.value.status == status, str(ei.value)
    assert all(w in str(ei.value) for w in words), str(ei.value)


@pytest.mark.gpu
def test_refusals_and_the_empty_list(eng, oracle):
    """MLGPU_ERR_INVALID without the reserve, from process_listed on a graph with the switch, from process_listed_groups on a graph
    without, while recording a sequence and with misaligned peaks - nothing is launched, the outputs keep their guard words; an empty
    list returns OK and writes nothing."""
    case, L, sums = synth(oracle), LISTS["k80"], {0: 16}
    K = L.size
    d_in, d_ctl = signals(eng, case, 0, 1, Layout.QUAD)
    d_out = [guarded(eng, K * 64, 0), guarded(eng, K * 64, 0)]
    d_peak = guarded(eng, K + 1, 0)
    g = build_group_graph(eng, case, sums)
    load_tables(g, case)
    g.set_voice_list(L)      # (a list without the groups reserve: no plan)
    assert g.listed_groups.size == 0
    refused(Status.ERR_INVALID, ["graph_process_listed_groups", "mlgpu_graph_reserve_voice_list_groups"], g.process_listed_groups, 1, d_in, d_out, d_controls=d_ctl, d_peak=d_peak)
    g.reserve_voice_list_groups(K)      # (the list in force gets its plan here)
    assert g.listed_groups.size == expected_plan("k80", 16)[2]
    refused(Status.ERR_INVALID, ["graph_process_listed:", "mlgpu_graph_process_listed_groups"], g.process_listed, 1, d_in, d_out, d_controls=d_ctl, d_peak=d_peak)
    refused(Status.ERR_INVALID, ["graph_process_listed_groups", "misaligned peaks"], g.process_listed_groups, 1, d_in, d_out, d_controls=d_ctl, d_peak=d_peak.ptr + 2)
    with eng.record():
        refused(Status.ERR_INVALID, ["graph_process_listed_groups", "recording a sequence"], g.process_listed_groups, 1, d_in, d_out, d_controls=d_ctl, d_peak=d_peak)
    off = build_group_graph(eng, case, {}, switch=False, voice_lists=True)
    off.set_voice_list(L)
    refused(Status.ERR_INVALID, ["graph_process_listed_groups", "mlgpu_graph_enable_voice_list_groups"], off.process_listed_groups, 1, d_in, d_out, d_controls=d_ctl, d_peak=d_peak)
    refused(Status.ERR_INVALID, ["graph_reserve_voice_list_groups", "mlgpu_graph_enable_voice_list_groups"], off.reserve_voice_list_groups, K)
    off.close()
    before = read_tables(g, case)
    g.set_voice_list(LISTS["empty"])
    assert g.voice_list_size == 0 and g.listed_groups.size == 0
    g.process_listed_groups(1, d_in, d_out, d_controls=d_ctl, d_peak=d_peak)
    after = read_tables(g, case)
    g.close()
    for d in d_out + [d_peak]:
        assert (d.download(np.uint32) == GUARD).all(), "a refused call or the call with an empty list wrote to an output or to the peaks"
    for key in before:
        assert_bits_equal(after[key], before[key], False, f"{key} after the refused calls and the empty list")
