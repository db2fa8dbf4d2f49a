"""Voice lists for graphs with sector delay rings on the device (mlgpu_graph_enable_voice_list_rings): the listed kernel of a ring
graph in ring layouts 1 and 4 - a listed call behaves as a graph of K voices made of voices L[0] ... L[K-1], ring words included, and
nobody else is touched.

Expected values: ring memory cannot be read back, so the expected value is a plain K-voice graph of the same description on the same
device, from clear with the gathered tables and inputs (test_gpu_graph_voice_list.py: check_rings) - in ring layout 0, which the
existing graph tests pin to the oracle: the project's rule is the same results in every layout. Each such reference is computed once
and shared by the layouts' cases. All comparisons are bit-exact.

V = 2352, T = 3. ring_case's delay times (1 to 95 samples) lie on both sides of layout 4's 16-sample history boundary."""
import types

import numpy as np
import pytest

import graph_voice_list_cases as cases
from graph_voice_list_cases import LISTS, T, V, build_graph, expected_peaks, gathered, load_tables
from graph_voice_list_groups_cases import build_group_graph
from inputs import assert_bits_equal, lcg_noise
from madronalib_amd.constants import Proc, Status
from test_gpu_graph_voice_list import check_peaks, read_tables, refused, run_listed, run_plain
from test_gpu_graph_voice_list_groups import run_groups

LANE_CLOCK = "#define MLGPU_RING_LANE_CLOCK"
_cases, _refs = {}, {}


@pytest.fixture(scope="module")
def eng():
    import madronalib_amd as ml
    e = ml.Engine(0)
    yield e
    e.close()


def pitchbend_case():
    """One PitchbendableDelay on a streamed input, its delay time a per-voice param (two rings; layout 4 writes and reads one)."""
    desc = [dict(name="x", type="input"), dict(name="dt", type="param"),
            dict(name="pb", type="proc", kind=Proc.PITCHBENDABLE_DELAY, inputs=["x", "dt"], max_delay=180.0)]
    rng = np.random.default_rng(97)
    return types.SimpleNamespace(desc=desc, outputs=["pb"], mix=(), inputs={"x": lcg_noise(np.arange(V, dtype=np.uint32) + 333, 64 * T)}, groups={}, controls={},
                                 params={"dt": rng.uniform(1.0, 95.0, V).astype(np.float32)}, coeffs={}, states=None)


def case_of(which):
    if which not in _cases:
        _cases[which] = pitchbend_case() if which == "pitchbend" else cases.ring_case(which)
    return _cases[which]


def window(case, t0, n):
    """The case with its inputs cut to DSPVectors [t0, t0 + n)."""
    return types.SimpleNamespace(**{**vars(case), "inputs": {k: np.ascontiguousarray(a[:, 64 * t0:64 * (t0 + n)]) for k, a in case.inputs.items()}})


def ring_graph(eng, case, layout, rings=True):
    """The case's V-voice graph with voice lists in ring layout `layout`, compiled."""
    g = build_graph(eng, case, V, True, layout, compile_now=False)
    if rings:
        g.enable_voice_list_rings()
    g.compile()
    assert g.delay_layout == (4 if layout == 3 else layout)
    return g


def k_reference(eng, which, L, t0=0, n=T, state=None, key=None):
    """A plain graph of the K voices L of the case, ring layout 0, from clear, run for DSPVectors [t0, t0 + n): (outputs [K][64 n], its
    tables). state: {(node, word): [K] uint32} set before the run. key: computed once per key."""
    if key is not None and key in _refs:
        return _refs[key]
    k = gathered(case_of(which), L)
    gk = build_graph(eng, k, L.size, voice_lists=False)
    load_tables(gk, k)
    for (node, word), values in (state or {}).items():
        gk.set_state(node, word, values)
    outs = run_plain(eng, gk, window(k, t0, n), L.size, n)
    tables = read_tables(gk, k)
    gk.close()
    for y in outs:
        y.setflags(write=False)
    if key is not None:
        _refs[key] = (outs, tables)
    return outs, tables


def launch(eng, g, case, K, t0, n):
    """One listed launch of DSPVectors [t0, t0 + n) with the list in force: (outputs, peaks [K])."""
    outs, peaks = run_listed(eng, g, window(case, t0, n), K, [n])
    return outs, peaks[0]


# ---- the one rule, in both layouts ------------------------------------------------------------------------------------------------------
def check_rings(eng, which, layout, lname):
    case, L = case_of(which), LISTS[lname]
    what = f"{which} layout={layout} list={lname}"
    C = np.setdiff1d(np.arange(V), L).astype(np.uint32)
    g = ring_graph(eng, case, layout)
    load_tables(g, case)
    g.set_voice_list(L)
    before = read_tables(g, case)
    got, peaks = run_listed(eng, g, case, L.size, [1, T - 1])      # (launches of 1 + 2 against the K-voice graph's one launch)
    after = read_tables(g, case)
    want, want_tables = k_reference(eng, which, L, key=(which, lname))
    for o in range(len(case.outputs)):
        assert np.abs(want[o]).max() > 1e-3
        assert_bits_equal(got[o], want[o], True, f"{what}: output {o} against a {L.size}-voice graph")
    check_peaks(peaks, want, [1, T - 1], what)
    for key in before:
        assert_bits_equal(after[key][:, L], want_tables[key], False, f"{what}: {key} of the listed voices against the {L.size}-voice graph")
        assert_bits_equal(after[key][:, C], before[key][:, C], False, f"{what}: {key} of the unlisted voices against the download before the call")
    if C.size:
        # the complement, on the same graph: its rings were not touched and no time has passed for it - a C-voice graph from clear
        g.set_voice_list(C)
        got_c, _ = run_listed(eng, g, case, C.size, [T])
        want_c, tables_c = k_reference(eng, which, C, key=(which, lname, "complement"))
        for o in range(len(case.outputs)):
            assert_bits_equal(got_c[o], want_c[o], True, f"{what}: output {o} of the complement against a {C.size}-voice graph from clear")
        final = read_tables(g, case)
        for key in before:
            assert_bits_equal(final[key][:, C], tables_c[key], False, f"{what}: {key} of the complement")
            assert_bits_equal(final[key][:, L], after[key][:, L], False, f"{what}: {key} of the first list after the complement ran")
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lname", ["k80", "k2100", "all"])
@pytest.mark.parametrize("layout", [1, 4])
def test_string_graph_listed(eng, layout, lname):
    """input -> FractionalDelay (per-voice delay time) -> OnePole -> gain -> back in through a feedback node: outputs, peaks and tables
    of the listed voices against the K-voice graph, tables of the unlisted voices against the download before, then the complement
    against a graph from clear."""
    check_rings(eng, "string", layout, lname)


@pytest.mark.gpu
@pytest.mark.parametrize("lname", ["k80", "all"])
@pytest.mark.parametrize("layout", [1, 4])
def test_three_ring_graph_listed(eng, layout, lname):
    """Three delay nodes in series: layout 4 issues the three rings' loads together in the trip's prologue, each lane its own voice's."""
    check_rings(eng, "three", layout, lname)


@pytest.mark.gpu
def test_layout_3_resolves_to_the_sector_trips(eng):
    """Layout 3 under the switch: layout 4 for the one-ring string (2 without voice lists), in both kernels; and the listed launch runs."""
    case, L = case_of("string"), LISTS["k80"]
    g = ring_graph(eng, case, 3)
    assert g.delay_layout == 4 and "#define MLGPU_RING_WINDOWS 3\n" in g.source and LANE_CLOCK in g.listed_source() and LANE_CLOCK not in g.source
    load_tables(g, case)
    g.set_voice_list(L)
    got, _ = run_listed(eng, g, case, L.size, [T])
    g.close()
    want, _ = k_reference(eng, "string", L, key=("string", "k80"))
    assert_bits_equal(got[0], want[0], True, "layout 3: the listed output against an 80-voice graph")


# ---- write indices that differ by voice ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["1", "4", "4-strict"])
def test_write_indices_that_differ_by_voice(eng, monkeypatch, form):
    """List A (every second entry of k80) for one DSPVector, then k80 for two: in the second launch the voices of A are 64 samples ahead
    of their neighbours. Voices of A against an |A|-voice graph run for 3 DSPVectors, the others against a graph run for 2 on the inputs
    of DSPVectors 1 and 2. Layout 4 takes its trips on each lane's clock (the generated source says so); 4-strict is the same kernel
    with the plain kernel's aligned test (MLGPU_GRAPH_RING_LANE_CLOCK=0: sample by sample through memory for such a wavefront)."""
    layout = int(form[0])
    if form == "4-strict":
        monkeypatch.setenv("MLGPU_GRAPH_RING_LANE_CLOCK", "0")
    case, L = case_of("string"), LISTS["k80"]
    in_a = np.arange(L.size) % 2 == 0
    A, B = L[in_a], L[~in_a]
    g = ring_graph(eng, case, layout)
    assert (LANE_CLOCK in g.listed_source()) == (form == "4")
    load_tables(g, case)
    g.set_voice_list(A)
    (first,), peak1 = launch(eng, g, case, A.size, 0, 1)
    g.set_voice_list(L)
    (second,), peak2 = launch(eng, g, case, L.size, 1, 2)
    tables = read_tables(g, case)
    g.close()
    (want_a,), tables_a = k_reference(eng, "string", A, 0, 3, key=("string", "A", 3))
    (want_b,), tables_b = k_reference(eng, "string", B, 1, 2, key=("string", "B", 2))
    assert np.abs(want_a).max() > 1e-3 and np.abs(want_b).max() > 1e-3
    assert_bits_equal(first, want_a[:, :64], True, f"{form}: list A's DSPVector")
    assert_bits_equal(second[in_a], want_a[:, 64:], True, f"{form}: the voices of A in the second launch, one DSPVector ahead")
    assert_bits_equal(second[~in_a], want_b, True, f"{form}: the other voices in the second launch")
    assert_bits_equal(peak1, expected_peaks([want_a[:, :64]]), False, f"{form}: peaks of list A")
    assert_bits_equal(peak2[in_a], expected_peaks([want_a[:, 64:]]), False, f"{form}: peaks of the voices of A in the second launch")
    assert_bits_equal(peak2[~in_a], expected_peaks([want_b]), False, f"{form}: peaks of the other voices")
    for key in tables:
        assert_bits_equal(tables[key][:, A], tables_a[key], False, f"{form}: {key} of the voices of A")
        assert_bits_equal(tables[key][:, B], tables_b[key], False, f"{form}: {key} of the other voices")
    wi = tables[("state", "line")][0]
    assert (wi[A] == 192).all() and (wi[B] == 128).all()


@pytest.mark.gpu
def test_one_voice_off_a_sector_boundary(eng):
    """Layout 4, one listed voice's write index set to 3 before the first launch: its wavefront goes sample by sample through memory.
    Against an 80-voice graph with the same state word."""
    case, L = case_of("string"), LISTS["k80"]
    pos = 37
    g = ring_graph(eng, case, 4)
    load_tables(g, case)
    wi = np.zeros(V, np.uint32)
    wi[L[pos]] = 3
    g.set_state("line", 0, wi)
    g.set_voice_list(L)
    got, peaks = run_listed(eng, g, case, L.size, [1, T - 1])
    tables = read_tables(g, case)
    g.close()
    wk = np.zeros(L.size, np.uint32)
    wk[pos] = 3
    want, want_tables = k_reference(eng, "string", L, state={("line", 0): wk})
    assert want_tables[("state", "line")][0, pos] == 3 + 64 * T
    assert_bits_equal(got[0], want[0], True, "one voice out of line: the output against an 80-voice graph with the same write index")
    check_peaks(peaks, want, [1, T - 1], "one voice out of line")
    for key in tables:
        assert_bits_equal(tables[key][:, L], want_tables[key], False, f"one voice out of line: {key}")


# ---- spare lanes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", [1, 4])
def test_spare_lanes_of_a_mixed_down_output(eng, oracle, layout):
    """The string's output mixed down, list k80: the second wavefront's 48 spare lanes run the last listed voice again, on its ring
    memory. The mixdown against oracle.mixdown of the 80-voice graph's rows, every table word of the listed voices - the last one's
    among them - against that graph."""
    base, L = case_of("string"), LISTS["k80"]
    case = types.SimpleNamespace(**{**vars(base), "mix": (0,)})
    g = ring_graph(eng, case, layout)
    g.reserve_mixdown(T)
    load_tables(g, case)
    g.set_voice_list(L)
    before = read_tables(g, case)
    got, peaks = run_listed(eng, g, case, L.size, [1, T - 1])
    tables = read_tables(g, case)
    g.close()
    want, want_tables = k_reference(eng, "string", L, key=("string", "k80"))
    assert_bits_equal(got[0], oracle.mixdown(np.ascontiguousarray(want[0]), None), True, f"layout {layout}: the mixdown against the 80-voice graph's rows")
    check_peaks(peaks, want, [1, T - 1], f"layout {layout}, mixed down")
    rest = np.setdiff1d(np.arange(V), L)
    for key in tables:
        assert_bits_equal(tables[key][:, L], want_tables[key], False, f"layout {layout}, mixed down: {key} of the listed voices")
        assert_bits_equal(tables[key][:, L[-1]], want_tables[key][:, -1], False, f"layout {layout}, mixed down: {key} of the last listed voice")
        assert_bits_equal(tables[key][:, rest], before[key][:, rest], False, f"layout {layout}, mixed down: {key} of the unlisted voices")


# ---- PitchbendableDelay -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", [4, 1])
def test_pitchbendable_delay_listed(eng, layout):
    """One PitchbendableDelay with a per-voice delay time, from clear, k80: layout 4 keeps one ring for both cores where a lane's two
    write indices agree - a question each lane answers for itself."""
    case, L = case_of("pitchbend"), LISTS["k80"]
    g = ring_graph(eng, case, layout)
    load_tables(g, case)
    g.set_voice_list(L)
    before = read_tables(g, case)
    got, peaks = run_listed(eng, g, case, L.size, [1, T - 1])
    tables = read_tables(g, case)
    g.close()
    want, want_tables = k_reference(eng, "pitchbend", L, key=("pitchbend", "k80"))
    assert np.abs(want[0]).max() > 1e-3
    assert_bits_equal(got[0], want[0], True, f"PitchbendableDelay layout {layout}: the output against an 80-voice graph")
    check_peaks(peaks, want, [1, T - 1], f"PitchbendableDelay layout {layout}")
    rest = np.setdiff1d(np.arange(V), L)
    for key in tables:
        assert_bits_equal(tables[key][:, L], want_tables[key], False, f"PitchbendableDelay layout {layout}: {key} of the listed voices")
        assert_bits_equal(tables[key][:, rest], before[key][:, rest], False, f"PitchbendableDelay layout {layout}: {key} of the unlisted voices")


def pitchbend_history(eng, layout):
    """A PitchbendableDelay bank with HISTORY: three listed launches of one DSPVector with a fresh random half of the voices each (write
    indices 0, 64, 128 or 192 afterwards, ring 0 alone written in layout 4), all voices listed for one DSPVector, then one voice of k80's
    first wavefront moved 3 samples off its sector boundary - both of its cores, so its two write indices still agree - and k80 for two
    DSPVectors: in layout 4 that wavefront leaves the trips with 63 voices whose samples live in ring 0 alone. Returns every launch's
    output and peaks and the tables at the end; in layout 4 also asks for mlgpu_graph_process after the rotation, which is refused."""
    case, L = case_of("pitchbend"), LISTS["k80"]
    g = ring_graph(eng, case, layout, rings=bool(layout))
    g.reserve_voice_list(V)
    load_tables(g, case)
    rng = np.random.default_rng(2024)
    results = []
    for t in range(3):
        half = np.sort(rng.choice(V, V // 2, replace=False)).astype(np.uint32)
        g.set_voice_list(half)
        results.append(launch(eng, g, case, half.size, t, 1))
    indices = g.get_state("pb", 0)
    assert (indices == g.get_state("pb", 5)).all() and np.unique(indices).size == 4 and np.unique(indices[L[:64]]).size > 1
    if layout == 4:
        d_x, d_y = eng.to_device(np.ascontiguousarray(case.inputs["x"][:, :64])), eng.alloc(4 * V * 64)
        refused(Status.ERR_UNSUPPORTED, ["graph_process", "PitchbendableDelay", "delay layout 4", "after a listed launch", "mlgpu_graph_process_listed", "mlgpu_graph_clear"],
                g.process, 1, [d_x], [d_y])
    g.set_voice_list(np.arange(V, dtype=np.uint32))
    results.append(launch(eng, g, case, V, 0, 1))
    for word in (0, 5):
        w = g.get_state("pb", word)
        w[L[37]] += 3
        g.set_state("pb", word, w)
    g.set_voice_list(L)
    results.append(launch(eng, g, case, L.size, 1, 2))
    tables = read_tables(g, case)
    if layout == 4:     # ... and after a clear the plain kernel runs again
        g.clear()
        g.process(1, [d_x], [d_y])
    g.close()
    return results, tables


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["4", "4-strict"])
def test_pitchbendable_delay_with_history(eng, monkeypatch, form):
    """Voices that have run in the trips (one ring for both cores) gathered into a wavefront that cannot: each lane still reads the ring
    its samples are in. Every launch of the sequence, and the tables after it, against the same sequence in ring layout 0, bit for bit.
    4-strict: the listed kernel with the plain kernel's aligned test - every wavefront of the rotated bank is outside the trips.
    (Layout 4 only: layout 1 always keeps two rings. And a write index moved AFTER history is outside what layout 1 promises - the three
    positions skipped hold other stale samples there than in the rows, in the plain kernel as well.)"""
    if form == "4-strict":
        monkeypatch.setenv("MLGPU_GRAPH_RING_LANE_CLOCK", "0")
    results, tables = pitchbend_history(eng, int(form[0]))
    monkeypatch.delenv("MLGPU_GRAPH_RING_LANE_CLOCK", raising=False)
    if "pitchbend history" not in _refs:
        _refs["pitchbend history"] = pitchbend_history(eng, 0)
    want, want_tables = _refs["pitchbend history"]
    for k, ((outs, peaks), (outs0, peaks0)) in enumerate(zip(results, want)):
        assert np.abs(outs0[0]).max() > 1e-3
        assert_bits_equal(outs[0], outs0[0], True, f"PitchbendableDelay with history, {form}: launch {k} against layout 0")
        assert_bits_equal(peaks, peaks0, False, f"PitchbendableDelay with history, {form}: peaks of launch {k} against layout 0")
    for key in want_tables:
        assert_bits_equal(tables[key], want_tables[key], False, f"PitchbendableDelay with history, {form}: {key} against layout 0")


# ---- the lane plan ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lane_plan_next_to_rings(eng):
    """The string graph with its output summed by instruments of 16 voices, the listed form by the lane plan, k80: ring layouts 1 and 4
    under the switch against the same graph in layout 0 - the summed rows, the peaks, every table. (The plan's pads leave before the
    rings' first ballot.)"""
    case, L = case_of("string"), LISTS["k80"]
    results = {}
    for layout in (1, 4, 0):
        g = build_group_graph(eng, case, {0: 16}, delay_windows=layout, compile_now=False)
        if layout:
            g.enable_voice_list_rings()
        g.compile()
        assert g.delay_layout == layout and "a.lanePlan" in g.listed_source() and ("ldsRings" in g.listed_source()) == bool(layout)
        load_tables(g, case)
        g.reserve_voice_list_groups(L.size)
        g.set_voice_list(L)
        J = g.listed_groups.size
        outs, peaks = run_groups(eng, g, case, {0: 16}, L.size, J, [1, T - 1])
        results[layout] = (outs, peaks, read_tables(g, case))
        g.close()
    outs0, peaks0, tables0 = results[0]
    assert J == np.unique(L // 16).size and outs0[0].shape == (J, 64 * T) and np.abs(outs0[0]).max() > 1e-3
    for layout in (1, 4):
        outs, peaks, tables = results[layout]
        assert_bits_equal(outs[0], outs0[0], True, f"the lane plan's group sums: layout {layout} against layout 0")
        for a, b in zip(peaks, peaks0):
            assert_bits_equal(a, b, False, f"the lane plan's peaks: layout {layout} against layout 0")
        for key in tables0:
            assert_bits_equal(tables[key], tables0[key], False, f"the lane plan: {key}, layout {layout} against layout 0")


# ---- a voice steal with a list in force -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", [1, 4])
def test_clear_rings_with_a_list_in_force(eng, layout):
    """k80 for one DSPVector; Update.clear_rings of a listed voice and of an unlisted one; k80 again; then k80 and the unlisted voice.
    The listed voice goes on as a voice from silence (a one-voice graph from clear on DSPVectors 1 and 2), the unlisted voice's first
    run is a voice from clear; and the whole sequence gives the bits of the same sequence in ring layout 0."""
    import madronalib_amd as ml
    case, L = case_of("string"), LISTS["k80"]
    a_pos = 70                                                     # (in the list's second, partial wavefront)
    a = int(L[a_pos])
    rest = np.setdiff1d(np.arange(V), L)
    u = int(rest[(rest > 1000) & (case.params["dt"][rest] > 17.0) & (case.params["dt"][rest] < 40.0)][0])   # (it sounds within its first DSPVector)
    L2 = np.sort(np.append(L, np.uint32(u))).astype(np.uint32)
    u_pos = int(np.searchsorted(L2, u))
    results = []
    for lay in (layout, 0):
        g = ring_graph(eng, case, lay, rings=bool(lay))
        load_tables(g, case)
        g.reserve_voice_list(L2.size)
        g.reserve_updates(4096)
        g.set_voice_list(L)
        (y0,), _ = launch(eng, g, case, L.size, 0, 1)
        g.apply_updates([ml.Update.clear_rings(-1, a, 1), ml.Update.clear_rings(-1, u, 1)])
        (y1,), _ = launch(eng, g, case, L.size, 1, 1)
        g.set_voice_list(L2)
        (y2,), _ = launch(eng, g, case, L2.size, 2, 1)
        results.append((y0, y1, y2, read_tables(g, case)))
        g.close()
    (y0, y1, y2, tables), (z0, z1, z2, tables0) = results
    for k, (y, z) in enumerate(((y0, z0), (y1, z1), (y2, z2))):
        assert_bits_equal(y, z, True, f"layout {layout} against layout 0: launch {k}")
    for key in tables0:
        assert_bits_equal(tables[key], tables0[key], False, f"layout {layout} against layout 0: {key}")
    (want_a,), _ = k_reference(eng, "string", np.array([a], np.uint32), 1, 2, key=("string", "stolen"))
    (want_u,), _ = k_reference(eng, "string", np.array([u], np.uint32), 2, 1, key=("string", "unlisted"))
    a_pos2 = int(np.searchsorted(L2, a))
    assert np.abs(want_a).max() > 1e-3 and np.abs(want_u).max() > 1e-3
    assert_bits_equal(np.concatenate([y1[a_pos], y2[a_pos2]]), want_a[0], True, f"layout {layout}: the cleared listed voice against a voice from silence")
    assert_bits_equal(y2[u_pos], want_u[0], True, f"layout {layout}: the cleared unlisted voice's first run against a voice from clear")


# ---- statuses -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_graph_made_without_the_switch_answers_as_before(eng):
    case = case_of("string")
    g = build_graph(eng, case, V, True, 1, compile_now=False)
    refused(Status.ERR_UNSUPPORTED, ["voice lists", "delay layout 1", "mlgpu_graph_set_delay_layout(g, 0)"], g.compile)
    g.close()
    g = build_graph(eng, case, V, False, 4)
    refused(Status.ERR_INVALID, ["graph_set_voice_list", "mlgpu_graph_enable_voice_lists", "before compile"], g.set_voice_list, [1, 2, 3])
    refused(Status.ERR_INVALID, ["graph_process_listed", "mlgpu_graph_enable_voice_lists"], g.process_listed, T, [0], [0])
    refused(Status.ERR_INVALID, ["graph_enable_voice_list_rings", "before mlgpu_graph_compile"], g.enable_voice_list_rings)
    g.close()
    g = ring_graph(eng, case, 1)
    refused(Status.ERR_INVALID, ["graph_process_listed_groups", "mlgpu_graph_enable_voice_list_groups"], g.process_listed_groups, T, [0], [0])
    g.close()
