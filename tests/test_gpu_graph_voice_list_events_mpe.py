"""Voice lists for graphs with event rows under the MPE protocol, on the device (mlgpu_graph_enable_voice_list_mpe_events,
mlgpu_events_sounding_graph_voices): the listed kernels around mlev::CtlVoiceMpe / CtlRowsMpe of the gathered voice.

THE COMPARATOR is made of existing calls only, as in tests/test_gpu_graph_voice_list_events.py: a twin MPE events object fed the same
events, mlgpu_events_process writing the seven rows of all V voices, a twin graph with those rows as streamed inputs, process_listed /
process_listed_groups with the same lists. This is HIP against HIP, one step from the reference: tests/test_gpu_events.py (scenario mpe5)
pins e2s_kernel to the reference's class, tests/test_gpu_graph_voice_list*.py pin the listed graph calls to the oracle. Every comparison
is bitwise. Shapes, performances and the events objects' setup are those of tests/test_gpu_graph_events_mpe.py: 6 blocks of 512 frames
in launches of 3, 3 and 2 vectors.

THE GRAPH has the seven rows as source nodes, a OnePole on gate and one on z - state that follows the list - and either the seven rows
and the two filters' sum as outputs ("rows") or the in-order sum of the seven rows, for the mixdown and the group sums, and the two
filters ("sum").

Voice lists are strictly ascending (mlgpu_graph_set_voice_list refuses any other), so a list cannot name an instrument's voices far
apart: the ragged list is a random 70 of 130 voices whose positions 63 and 64 - two wavefronts - are voices of one instrument."""
import ctypes

import numpy as np
import pytest

from inputs import assert_bits_equal
from test_gpu_events import eng, gpu_run, performance  # noqa: F401  (eng: the module's engine fixture)
from test_gpu_graph_events_mpe import (BLOCK, CTRL, LAUNCHES, N_BLOCKS, ROW_NAMES, SEED0, SHAPES, add_block, config, make_events, mpe_performance,
                                       one_frame_gate_gaps, shape_instruments)
from test_gpu_graph_voice_list_events import tails_lists

pytestmark = pytest.mark.gpu
MAX_T = 3
GUARD = 0x7FC0ABCD     # a NaN no kernel writes
RAGGED = np.sort(np.random.default_rng(155).choice(130, 70, replace=False)).astype(np.uint32)


def graph_desc(fused, kind):
    import madronalib_amd as ml
    from madronalib_amd.constants import Op
    src = (lambda n, r: dict(name=n, type="event_row", kind=r)) if fused else (lambda n, r: dict(name=n, type="input"))
    d = [src(n, r) for r, n in enumerate(ROW_NAMES)]
    d += [dict(name="lpg", type="proc", kind=ml.Proc.ONE_POLE, inputs=["gate"]), dict(name="lpz", type="proc", kind=ml.Proc.ONE_POLE, inputs=["z"])]
    if kind == "rows":
        d.append(dict(name="st", type="op", kind=Op.ADD, inputs=["lpg", "lpz"]))
        return d, list(ROW_NAMES) + ["st"]
    acc = "pitch"      # (((((pitch + gate) + vox) + z) + x) + y) + mod
    for i, n in enumerate(ROW_NAMES[1:]):
        d.append(dict(name=f"s{i}", type="op", kind=Op.ADD, inputs=[acc, n]))
        acc = f"s{i}"
    return d, [acc, "lpg", "lpz"]


def row_sum(rows):
    s = rows[0]
    for r in range(1, 7):
        s = (s + rows[r]).astype(np.float32)
    return s


class Rig:
    """An events object and a graph over its voices. fused: the graph makes the seven rows itself and runs its listed events form; else
    the comparator: mlgpu_events_process writes the rows of all voices, the twin graph reads them, process_listed[_groups]."""

    def __init__(self, eng, cfg, N, fused, kind="rows", group=0, mix=False, switches=None, reserve=MAX_T):
        import madronalib_amd as ml
        self.eng, self.fused, self.N, self.P, self.V = eng, fused, N, cfg["polyphony"], N * cfg["polyphony"]
        self.group, self.mix = group, mix
        V = self.V
        self.ev = make_events(eng, cfg, N)
        desc, outs = graph_desc(fused, kind)
        if switches is None:
            switches = dict(voice_list_mpe_events=True) if fused else dict(voice_lists=True)
        g = ml.Graph(eng, V, desc, outs, output_groups={0: group} if group else None, compile_now=False, voice_list_groups=bool(group), **switches)
        if mix:
            g.set_output_mixdown(0, True)
        g.compile()
        self.g = g
        self.reset_graph()
        if fused:
            if switches.get("voice_list_mpe_events"):
                assert "mlev::CtlVoiceMpe ev_0;" in g.listed_source() and "mlev::CtlRowsMpe<124u> er_0;" in g.listed_source() and not g.inputs
            g.bind_events(self.ev)
            if reserve:
                self.ev.reserve_for_graph(reserve, rows=range(7))
        if group:
            g.reserve_voice_list_groups(V)
        else:
            g.reserve_voice_list(V)
        if mix:
            g.reserve_mixdown(MAX_T)
        self.g, self.n_out = g, len(outs)
        self.words = V * MAX_T * 64 + 16
        self.d_out = [eng.alloc(4 * self.words) for _ in range(self.n_out)]
        self.d_peak = eng.alloc(4 * (V + 16))
        self.rows = [eng.alloc(4 * V * MAX_T * 64) for _ in range(8)]

    def reset_graph(self):
        """The graph's state cleared (the events object's clear does not reach it), the two filters' coefficients set."""
        import madronalib_amd as ml
        self.g.clear()
        for p, k in (("lpg", 0.15), ("lpz", 0.05)):
            self.g.set_coeffs(p, [np.full(self.V, c, np.float32) for c in np.atleast_1d(ml.OnePole.makeCoeffs(k))])

    def add_block(self, instruments, b):
        add_block(self.ev, instruments, b)

    def sounding(self, T, off):
        self.ev.route_ahead(T, off)
        return self.ev.sounding_graph_voices()

    def state(self):
        return np.stack([self.g.get_state(p, i) for p in ("lpg", "lpz") for i in range(self.g.num_state(p))])

    def launch(self, T, off, L):
        """One launch with the list L. Returns (outputs - [rows][64 T] each, a mixed-down one [64 T] -, peaks [K], the comparator's seven
        rows [7][V][64 T] or None). Whatever lies behind an output's rows and behind the K peaks keeps its guard words."""
        from madronalib_amd.constants import Layout
        g, K = self.g, len(L)
        g.set_voice_list(L)
        guard = np.full(self.words, GUARD, np.uint32)
        for d in self.d_out:
            d.upload(guard)
        self.d_peak.upload(guard[:self.V + 16])
        rows = None
        if self.fused:
            call = g.process_events_listed_groups if self.group else g.process_events_listed
            call(T, off, [], self.d_out, out_layout=Layout.VOICE_MAJOR, d_peak=self.d_peak)
        else:
            self.ev.process(T, off, self.rows, Layout.VOICE_MAJOR)
            rows = np.stack([r.download(np.float32, self.V * T * 64).reshape(self.V, T * 64).copy() for r in self.rows[:7]])
            call = g.process_listed_groups if self.group else g.process_listed
            call(T, [self.rows[ROW_NAMES.index(nm)] for nm in g.inputs], self.d_out, in_layout=Layout.VOICE_MAJOR, out_layout=Layout.VOICE_MAJOR,
                 d_peak=self.d_peak)
        outs = []
        for o, d in enumerate(self.d_out):
            n = 1 if (self.mix and o == 0) else (len(g.listed_groups) if (self.group and o == 0) else K)
            if self.mix and o == 0 and K == 0:
                n = 1       # (the sum of no voices: +0.0, written)
            w = d.download(np.uint32, self.words)
            assert (w[n * T * 64:] == GUARD).all(), f"output {o}: words behind its {n} rows were written"
            outs.append(w[:n * T * 64].view(np.float32).reshape(n, T * 64).copy() if not (self.mix and o == 0) else w[:T * 64].view(np.float32).copy())
        peaks = self.d_peak.download(np.uint32, self.V + 16)
        assert (peaks[K:] == GUARD).all(), "peaks: more than K words were written"
        return outs, peaks[:K].copy(), rows

    def close(self):
        self.g.close()
        self.ev.close()


def run_pair(eng, cfg, instruments, make_list, kind="rows", group=0, mix=False, n_blocks=N_BLOCKS, check=None):
    """The fused rig and the comparator through the performance with the same lists. check(k, L, ya, yb, pa, pb, rows, what) per launch
    (default: every output and the peaks equal). Returns the per-launch records (L, sounding set, fused outputs, comparator's rows) and
    the two rigs (the caller closes them)."""
    N = len(instruments)
    a, b = Rig(eng, cfg, N, True, kind, group, mix), Rig(eng, cfg, N, False, kind, group, mix)
    log = []
    for blk in range(n_blocks):
        a.add_block(instruments, blk), b.add_block(instruments, blk)
        for T, off in LAUNCHES:
            s = a.sounding(T, off)
            L = make_list(s)
            ya, pa, _ = a.launch(T, off, L)
            yb, pb, rows = b.launch(T, off, L)
            what = f"block {blk} offset {off} K {len(L)}"
            if group:
                assert np.array_equal(a.g.listed_groups, b.g.listed_groups), what
            if check is None:
                for o in range(len(ya)):
                    assert_bits_equal(ya[o], yb[o], True, f"{what}: output {o}")
                assert_bits_equal(pa, pb, False, f"{what}: peaks")
            else:
                check(len(log), L, ya, yb, pa, pb, rows, what)
            log.append((L, s, ya, rows))
        a.ev.clear_events(), b.ev.clear_events()
    return log, a, b


def check_rows(pitch_exact):
    """The "rows" graph: rows 1..6 of every listed voice are the comparator's own rows at the list's voices, the stateful output is the
    twin's; the pitch row and the peaks (which see the pitch output) for the list positions pitch_exact(k, L) gives."""
    def check(k, L, ya, yb, pa, pb, rows, what):
        for r in range(1, 7):
            assert_bits_equal(ya[r], rows[r][L], True, f"{what}: row {ROW_NAMES[r]} of every listed voice vs mlgpu_events_process")
            assert_bits_equal(yb[r], rows[r][L], True, f"{what}: the twin's row {ROW_NAMES[r]}")
        assert_bits_equal(ya[7], yb[7], True, f"{what}: the two OnePoles' sum of every listed voice")
        at = pitch_exact(k, L)
        assert_bits_equal(ya[0][at], rows[0][L][at], True, f"{what}: the pitch row vs mlgpu_events_process")
        assert_bits_equal(pa[at], pb[at], False, f"{what}: peaks")
    return check


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_shape_with_the_hosts_lists(eng, name):
    """G = 8 straddling wavefronts, G = 32, no padding lane, seven padding lanes, G = 2. The list per launch is the host's:
    route_ahead, sounding_graph_voices(), united with the sets of the two launches before. Rows 1..6 and the stateful output are exact
    for every listed voice; the pitch row for every listed voice where the drift is 0, else for the voices listed in every launch so
    far."""
    cfg, instruments = shape_instruments(name)
    every = [None]
    n_pitch = [0]

    def lists():
        make = tails_lists()

        def f(s):
            L = make(s)
            every[0] = set(L.tolist()) if every[0] is None else every[0] & set(L.tolist())
            return L
        return f

    def pitch_exact(k, L):
        at = np.arange(len(L)) if cfg["drift"] == 0.0 else np.flatnonzero(np.isin(L, sorted(every[0])))
        n_pitch[0] += len(at)
        return at
    log, a, b = run_pair(eng, cfg, instruments, lists(), check=check_rows(pitch_exact))
    a.close(), b.close()
    sizes = [len(L) for L, _, _, _ in log]
    assert max(sizes) > 0 and len(set(sizes)) >= 2 and n_pitch[0] > 0
    assert max(np.abs(y[1]).max() for _, _, y, _ in log if y[1].size) > 0 and max(np.abs(y[3]).max() for _, _, y, _ in log if y[3].size) > 0


def test_ragged_and_remapped_list(eng):
    """P5_V130, drift 0.3, a constant list of 70 voices: two wavefronts, the second ragged with 6 voices, an instrument's voices on both
    sides of the wavefront boundary, instruments with one to five voices listed. Listed since clear: all seven rows are exact."""
    assert len(RAGGED) == 70 and RAGGED[63] // 5 == RAGGED[64] // 5 and set(np.bincount(RAGGED // 5).tolist()) >= {1, 2, 3, 4, 5}
    assert np.any(np.diff(RAGGED) > 1)       # remapped: a list position is not a voice index
    cfg, instruments = shape_instruments("P5_V130")
    log, a, b = run_pair(eng, cfg, instruments, lambda s: RAGGED, check=check_rows(lambda k, L: np.arange(len(L))))
    a.close(), b.close()
    assert any(np.any(rows[0][RAGGED][:, 1:] != rows[0][RAGGED][:, :-1]) for _, _, _, rows in log)


@pytest.mark.parametrize("K", [130, 70])
def test_mixdown_of_the_listed_voices_with_spare_lanes(eng, K):
    """P5_V130, the sum of the seven rows mixed down: 130 listed voices leave 62 spare lanes, 70 leave 58 - they run the list's last
    voice, its lane and its main lane, again. Against the twin's process_listed of the same mixed-down output, and against the oracle's
    mixdown of the comparator's rows taken by list position and added in the node order."""
    from cpu_checkers import Oracle
    cfg, instruments = shape_instruments("P5_V130")
    L = np.arange(130, dtype=np.uint32) if K == 130 else RAGGED
    loud = [0.0]

    def check(k, L_, ya, yb, pa, pb, rows, what):
        for o in range(3):
            assert_bits_equal(ya[o], yb[o], True, f"{what}: output {o}")
        assert_bits_equal(pa, pb, False, f"{what}: peaks")
        want = Oracle().mixdown(np.ascontiguousarray(row_sum(rows)[L_]), None)
        assert_bits_equal(ya[0], want, True, f"{what}: the mixdown vs the oracle's of the comparator's rows")
        loud[0] = max(loud[0], float(np.abs(want).max()))
    log, a, b = run_pair(eng, cfg, instruments, lambda s: L, kind="sum", mix=True, check=check)
    assert_bits_equal(a.state(), b.state(), False, "graph state")
    a.close(), b.close()
    assert loud[0] > 0


@pytest.mark.parametrize("name,group", [("P16_V80", 16), ("P8_V72", 4)])
def test_lane_plan(eng, name, group):
    """process_events_listed_groups with the host's lists against the twin's process_listed_groups: a group sum of 16 = polyphony
    (G = 32 lanes per instrument in the events object) and one of 4 under polyphony 8 (two groups per instrument, G = 16). The J rows of
    the groups' sums, listed_groups, the K rows of the plain outputs and the peaks."""
    cfg, instruments = shape_instruments(name)
    log, a, b = run_pair(eng, cfg, instruments, tails_lists(), kind="sum", group=group)
    assert_bits_equal(a.state(), b.state(), False, "graph state")
    a.close(), b.close()
    counts = set()       # listed voices per listed group: whole groups and partial ones occur
    for L, _, y, _ in log:
        assert y[0].shape[0] == len(np.unique(L // group)) and y[1].shape[0] == len(L)
        counts |= set(np.bincount(L // group).tolist()) - {0}
    assert group in counts and any(c < group for c in counts) and len({len(L) for L, _, _, _ in log}) >= 2
    assert max(np.abs(y[0]).max() for _, _, y, _ in log if y[0].size) > 0


def test_changing_lists_with_drift(eng):
    """P7_V70, drift 0.3: the host's lists, less every voice v % 7 == 3 in every fourth launch - voices leave and come back. Rows 1..6
    and the stateful output are exact from a relisted voice's first listed vector on; the pitch row for the voices never unlisted
    (voices 0, 8 and 69 are forced into every list)."""
    cfg, instruments = shape_instruments("P7_V70")
    always = np.array([0, 8, 69], np.uint32)
    make = tails_lists()
    n = [0]
    lists = []

    def make_list(s):
        L = np.union1d(make(s), always).astype(np.uint32)
        n[0] += 1
        if n[0] % 4 == 0:
            L = L[L % 7 != 3]
        lists.append(L)
        return L

    def pitch_exact(k, L):
        never_unlisted = [v for v in L.tolist() if all(v in Lk for Lk in lists)]
        return np.flatnonzero(np.isin(L, never_unlisted))
    log, a, b = run_pair(eng, cfg, instruments, make_list, check=check_rows(pitch_exact))
    a.close(), b.close()
    # on the lists themselves: some voice was listed, then not, then listed again; the forced voices never left
    sets = [set(L.tolist()) for L in lists]
    relisted = [v for v in range(70) if any(v in sets[i] and v not in sets[j] and v in sets[k] for i in range(len(sets)) for j in range(i + 1, len(sets))
                                             for k in range(j + 1, min(j + 4, len(sets))))]
    assert relisted and all(int(v) in s for s in sets for v in always)
    assert any(np.any(rows[0][always][:, 1:] != rows[0][always][:, :-1]) for _, _, _, rows in log)


def test_hand_over(eng):
    """P8_V72, drift 0: two listed blocks, then a block by process_events (all voices), then a block by mlgpu_events_process. Every row of
    every voice in the last two blocks has the bits of a twin object that only ever used mlgpu_events_process."""
    from madronalib_amd.constants import Layout
    cfg, instruments = shape_instruments("P8_V72", n_blocks=4)
    want = gpu_run(eng, cfg, instruments, BLOCK, 4, 3)
    r = Rig(eng, cfg, len(instruments), True)
    make = tails_lists()
    sizes = []
    for blk in range(2):
        r.add_block(instruments, blk)
        for T, off in LAUNCHES:
            L = make(r.sounding(T, off))
            sizes.append(len(L))
            y = r.launch(T, off, L)[0]
            at = slice(blk * BLOCK + off, blk * BLOCK + off + 64 * T)
            for row in range(7):
                assert_bits_equal(y[row], want[row][L][:, at], True, f"listed block {blk} offset {off}: row {ROW_NAMES[row]}")
        r.ev.clear_events()
    assert 0 < min(sizes) < r.V
    for blk, fused in ((2, True), (3, False)):
        r.add_block(instruments, blk)
        for T, off in LAUNCHES:
            if fused:
                r.g.process_events(T, off, [], r.d_out, out_layout=Layout.VOICE_MAJOR)
                got = [d.download(np.float32, r.V * T * 64).reshape(r.V, T * 64) for d in r.d_out[:7]]
            else:
                r.ev.process(T, off, r.rows, Layout.VOICE_MAJOR)
                got = [d.download(np.float32, r.V * T * 64).reshape(r.V, T * 64) for d in r.rows[:7]]
            at = slice(blk * BLOCK + off, blk * BLOCK + off + 64 * T)
            for row in range(7):
                assert_bits_equal(got[row], want[row][:, at], True, f"block {blk} ({'process_events' if fused else 'mlgpu_events_process'}) offset {off}: row {ROW_NAMES[row]}")
        r.ev.clear_events()
    r.close()
    assert np.abs(want[1][:, 2 * BLOCK:]).max() > 0 and len(np.unique(want[3][:, 2 * BLOCK:])) > 2


def test_protocol_at_run_time(eng):
    """One graph with all switches, bound to an object that goes MIDI -> MPE -> MIDI by configure(mpe=...) (which clears). Under MIDI the
    listed outputs are those of a graph built with voice_list_events alone on a MIDI twin; under MPE the comparator's. A reserve made at
    setup survives the switches: a block one vector longer gets ERR_RANGE in every protocol, with its events intact."""
    import madronalib_amd as ml
    from madronalib_amd.constants import Layout, Status
    P, N, n_blocks = 5, 6, 2
    # (every performance starts with an event on frame 0 - controller 1, which nothing follows: an instrument that has played stays awake
    # through mlgpu_events_set_protocol while a fresh twin wakes with its first event)
    wake = [(CTRL, 1, 1, 0, 0.0, 0.0)]
    midi = [wake + performance("midi", 100 * k + 10, BLOCK * n_blocks, P) for k in range(N)]
    midi2 = [wake + performance("midi", 100 * k + 11, BLOCK * n_blocks, P) for k in range(N)]
    mpe = [wake + mpe_performance(100 * k + SEED0, BLOCK * n_blocks, P, burst=(k % 3 == 0)) for k in range(N)]
    rig = Rig(eng, config(P, 0.0, mpe=0), N, True)

    def phase(instruments, twin, mpe_now):
        make = tails_lists()
        loud = 0.0
        for b in range(n_blocks):
            rig.add_block(instruments, b), twin.add_block(instruments, b)
            with pytest.raises(ml.MlgpuError) as ei:      # one vector more than the reserve: refused, nothing consumed
                rig.g.process_events_listed(MAX_T + 1, 0, [], rig.d_out, out_layout=Layout.VOICE_MAJOR, d_peak=rig.d_peak)
            assert ei.value.status == Status.ERR_RANGE, str(ei.value)
            for T, off in LAUNCHES:
                s = rig.sounding(T, off)
                if not mpe_now:
                    assert np.array_equal(s, rig.ev.sounding_voices())
                L = make(s)
                ya, pa, _ = rig.launch(T, off, L)
                yb, pb, _ = twin.launch(T, off, L)
                for o in range(8):
                    assert_bits_equal(ya[o], yb[o], True, f"{'MPE' if mpe_now else 'MIDI'} block {b} offset {off}: output {o}")
                assert_bits_equal(pa, pb, False, "peaks")
                loud = max(loud, float(np.abs(ya[1]).max()) if len(L) else 0.0)
            rig.ev.clear_events(), twin.ev.clear_events()
        twin.close()
        assert loud > 0

    assert rig.ev.graph_reserve_bytes(MAX_T, range(7)) == (16 + 512 + 260 * 4) * MAX_T * N * P
    twin = Rig(eng, config(P, 0.0, mpe=0), N, True, switches=dict(voice_list_events=True))
    assert "CtlVoiceMpe" not in twin.g.listed_source() and "mlev::CtlVoice ev_0;" in twin.g.listed_source()
    phase(midi, twin, False)
    rig.ev.configure(mpe=1), rig.reset_graph()
    assert rig.ev.graph_reserve_bytes(MAX_T, range(7)) == (16 + 512 + 260 * 4) * MAX_T * N * 8
    phase(mpe, Rig(eng, config(P, 0.0), N, False), True)
    rig.ev.configure(mpe=0), rig.reset_graph()
    phase(midi2, Rig(eng, config(P, 0.0, mpe=0), N, True, switches=dict(voice_list_events=True)), False)
    rig.close()


def test_unlisted_voices_are_not_touched_and_an_empty_list_advances_the_events(eng):
    """P8_V72, drift 0. Listed launches leave the graph state of unlisted voices as it was, and write K rows and K peaks (Rig.launch
    checks the guard words behind them in every test of this file). A block whose lists are empty launches no voice kernel and still
    advances the events object: the next listed block has the comparator's bits."""
    cfg, instruments = shape_instruments("P8_V72", n_blocks=4)
    V = 72
    L = np.array([1, 2, 9, 17, 18, 40, 63, 64, 71], np.uint32)
    unlisted = np.setdiff1d(np.arange(V), L)
    a, b = Rig(eng, cfg, 9, True), Rig(eng, cfg, 9, False)
    for r in (a, b):        # state words nothing of a clear would leave
        r.g.set_state("lpg", 0, np.linspace(0.01, 0.2, V).astype(np.float32).view(np.uint32))
        r.g.set_state("lpz", 0, np.linspace(0.3, 0.1, V).astype(np.float32).view(np.uint32))
    before = a.state()
    everyone, nobody = np.arange(V, dtype=np.uint32), np.zeros(0, np.uint32)
    check = check_rows(lambda k, L_: np.arange(len(L_)))
    gate_up = False
    for blk in range(4):
        a.add_block(instruments, blk), b.add_block(instruments, blk)
        for i, (T, off) in enumerate(LAUNCHES):
            Lk = [L, L, nobody, everyone][blk]
            a.ev.route_ahead(T, off)
            ya, pa, _ = a.launch(T, off, Lk)
            yb, pb, rows = b.launch(T, off, Lk)
            check(0, Lk, ya, yb, pa, pb, rows, f"block {blk} launch {i}")
            if blk < 3:
                assert_bits_equal(a.state()[:, unlisted], before[:, unlisted], False, "unlisted voices' state words")
            if blk == 2:
                assert ya[0].shape[0] == 0
                gate_up = gate_up or bool(np.abs(rows[1]).max() > 0)
        a.ev.clear_events(), b.ev.clear_events()
    assert gate_up       # nobody ran in the third block, and somebody's gate was up
    assert not np.array_equal(a.state()[:, L], before[:, L])
    assert_bits_equal(a.state(), b.state(), False, "graph state after listed, empty and full launches")
    a.close(), b.close()


def test_the_sounding_set_covers_every_gate(eng):
    """P5, 26 playing instruments and two with an empty performance, MPE: in every launch every voice whose comparator gate row is
    non-zero anywhere in it is in sounding_graph_voices(); the silent instruments' voices never are (an instrument that has seen no event
    is not awake), so the set of all voices would not pass; some voice is stolen. Then MIDI on the same object: the set is
    sounding_voices()'."""
    from madronalib_amd.constants import Layout
    cfg, instruments = shape_instruments("P5_V130")
    instruments = instruments[:13] + [[]] + instruments[13:] + [[]]
    N, P = len(instruments), 5
    V = N * P
    silent = set(range(13 * P, 14 * P)) | set(range(V - P, V))
    ev = make_events(eng, cfg, N)
    d = [eng.alloc(4 * V * MAX_T * 64) for _ in range(8)]
    gates, sizes = [], []
    for blk in range(N_BLOCKS):
        add_block(ev, instruments, blk)
        for T, off in LAUNCHES:
            ev.route_ahead(T, off)
            s = ev.sounding_graph_voices()
            assert np.all(np.diff(s.astype(np.int64)) > 0) and not (set(s.tolist()) & silent)
            ev.process(T, off, d, Layout.VOICE_MAJOR)
            assert np.array_equal(ev.sounding_graph_voices(), s)       # valid until the next route
            gate = d[1].download(np.float32, V * T * 64).reshape(V, T * 64).copy()
            assert np.all(np.isin(np.flatnonzero(np.any(gate != 0, axis=1)), s)), f"block {blk} offset {off}: a sounding voice is missing"
            gates.append(gate)
            sizes.append(len(s))
        ev.clear_events()
    gate = np.concatenate(gates, 1)
    assert sum(one_frame_gate_gaps(gate[k * P:(k + 1) * P]) for k in range(N)) > 0, "no voice is stolen"
    assert 0 < min(sizes) and max(sizes) <= V - 2 * P and len(set(sizes)) > 2
    ev.configure(mpe=0)
    midi = [performance("midi", 100 * k + 10, BLOCK * 2, P) if k % 14 != 13 else [] for k in range(N)]
    for blk in range(2):
        add_block(ev, midi, blk)
        for T, off in LAUNCHES:
            ev.route_ahead(T, off)
            s = ev.sounding_graph_voices()
            assert np.array_equal(s, ev.sounding_voices()) and not (set(s.tolist()) & silent)
            ev.process(T, off, d, Layout.VOICE_MAJOR)
            gate = d[1].download(np.float32, V * T * 64).reshape(V, T * 64)
            assert np.all(np.isin(np.flatnonzero(np.any(gate != 0, axis=1)), s))
        ev.clear_events()
    ev.close()


def test_statuses(eng):
    import madronalib_amd as ml
    from madronalib_amd.constants import Layout, Status
    cfg, instruments = shape_instruments("P8_V72", n_blocks=1)

    def refused(status, words, fn, *args, **kw):
        with pytest.raises(ml.MlgpuError) as ei:
            fn(*args, **kw)
        assert ei.value.status == status and all(w in str(ei.value) for w in words), str(ei.value)
    a, b = Rig(eng, cfg, 9, True), Rig(eng, cfg, 9, False)
    # the switch is a build call
    refused(Status.ERR_INVALID, ["graph_enable_voice_list_mpe_events", "before mlgpu_graph_compile"], a.g.enable_voice_list_mpe_events)
    a.add_block(instruments, 0), b.add_block(instruments, 0)
    L = np.arange(0, 72, 1, dtype=np.uint32)[np.arange(72) % 4 != 2]
    a.g.set_voice_list(L)
    kw = dict(out_layout=Layout.VOICE_MAJOR, d_peak=a.d_peak)
    state = a.state()
    guard = np.full(a.words, GUARD, np.uint32)
    for d in a.d_out:
        d.upload(guard)
    # process_listed on the events graph still names the events calls
    refused(Status.ERR_INVALID, ["graph_process_events_listed"], a.g.process_listed, 3, [], a.d_out, **kw)
    # longer than the reserve: ERR_RANGE before anything is consumed, by the listed call and by route_ahead
    refused(Status.ERR_RANGE, ["mlgpu_events_reserve_for_graph"], a.g.process_events_listed, MAX_T + 1, 0, [], a.d_out, **kw)
    refused(Status.ERR_RANGE, ["mlgpu_events_reserve_for_graph"], a.ev.route_ahead, MAX_T + 1, 0)
    refused(Status.ERR_INVALID, ["lane plan"], a.g.process_events_listed_groups, 3, 0, [], a.d_out, **kw)
    refused(Status.ERR_INVALID, ["negative"], a.g.process_events_listed, 3, -1, [], a.d_out, **kw)
    # sounding_graph_voices with too small a capacity: ERR_RANGE, the size reported, nothing written; sounding_voices stays refused
    s = a.sounding(3, 0)
    assert len(s) > 1
    n = ctypes.c_size_t(99)
    small = np.full(len(s), 0xDEAD, np.uint32)
    st = a.ev.L.mlgpu_events_sounding_graph_voices(a.ev.h, small.ctypes.data_as(ctypes.c_void_p), len(s) - 1, ctypes.byref(n))
    assert st == Status.ERR_RANGE and n.value == len(s) and (small == 0xDEAD).all()
    st = a.ev.L.mlgpu_events_sounding_graph_voices(a.ev.h, small.ctypes.data_as(ctypes.c_void_p), len(s), ctypes.byref(n))
    assert st == Status.OK and n.value == len(s) and np.array_equal(small, s)
    refused(Status.ERR_UNSUPPORTED, ["MIDI"], a.ev.sounding_voices)
    # other values than the routed launch's
    refused(Status.ERR_INVALID, ["mlgpu_events_route_ahead"], a.g.process_events_listed, 2, 0, [], a.d_out, **kw)
    for d in a.d_out:
        assert (d.download(np.uint32, a.words) == GUARD).all()
    assert_bits_equal(a.state(), state, False, "graph state after the refusals")
    # the next valid calls have the comparator's bits
    check = check_rows(lambda k, L_: np.arange(len(L_)))
    for i, (T, off) in enumerate(LAUNCHES):
        if i:
            a.ev.route_ahead(T, off)
        ya, pa, _ = a.launch(T, off, L)
        yb, pb, rows = b.launch(T, off, L)
        check(0, L, ya, yb, pa, pb, rows, f"after the refusals, offset {off}")
    assert np.abs(rows[1]).max() > 0
    a.close(), b.close()
    # a graph WITHOUT the new switch on an MPE object: today's refusal, the same status and words - it goes on to name the switch
    r = Rig(eng, cfg, 9, True, switches=dict(mpe_events=True, voice_list_events=True))
    assert "CtlVoiceMpe" not in r.g.listed_source()
    r.add_block(instruments, 0)
    r.g.set_voice_list(L)
    refused(Status.ERR_UNSUPPORTED, ["graph_process_events_listed", "MIDI", "mlgpu_graph_enable_voice_list_mpe_events"], r.g.process_events_listed, 3, 0, [], r.d_out,
            out_layout=Layout.VOICE_MAJOR, d_peak=r.d_peak)
    r.close()
