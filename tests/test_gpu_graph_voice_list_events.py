"""Voice lists for graphs with event rows on the device (mlgpu_graph_enable_voice_list_events, mlgpu_graph_process_events_listed[_groups],
mlgpu_events_route_ahead, mlgpu_events_sounding_voices).

THE COMPARATOR is made of existing calls only: fresh twin objects with the same events - mlgpu_events_process writing the pitch and gate
rows of all V voices, the twin graph with the two rows as streamed inputs, process_listed / process_listed_groups with the same lists.
HIP against HIP, one step from the reference, which tests/test_gpu_events.py pins (e2s_kernel against the reference's class; the
listed graph calls against the oracle in tests/test_gpu_graph_voice_list*.py). All comparisons are bitwise. Scenarios, performances
and the events objects' setup are those of tests/test_gpu_events.py."""
import numpy as np
import pytest

from inputs import assert_bits_equal
from test_gpu_events import SCENARIOS, eng, performance  # noqa: F401  (eng: the module's engine fixture)

pytestmark = pytest.mark.gpu
BLOCK, N_BLOCKS = 512, 8


def small_desc(event_rows):
    """pitch and gate as event rows (or, the twin, as streamed inputs): `p1` is the pitch row's own bits, `lp` a OnePole on the gate -
    gate-derived, with state -, `both` their sum."""
    import madronalib_amd as ml
    src = (lambda n, k: dict(name=n, type="event_row", kind=k)) if event_rows else (lambda n, k: dict(name=n, type="input"))
    return [src("gate", 1), src("pitch", 0), dict(name="one", type="const", value=1.0),
            dict(name="lp", type="proc", kind=ml.Proc.ONE_POLE, inputs=["gate"]),
            dict(name="p1", type="op", kind=ml.Op.MULTIPLY, inputs=["pitch", "one"]),
            dict(name="both", type="op", kind=ml.Op.ADD, inputs=["p1", "lp"])], ["p1", "lp", "both"]


class Rig:
    """An events object and a graph over its voices. fused: the graph makes the two rows itself and runs its listed events form;
    else the comparator: mlgpu_events_process writes the rows for all voices, the twin graph reads them, process_listed[_groups]."""

    def __init__(self, eng, cfg, N, fused, patch="small", group=0, mix=(), max_vectors=8, switch=True, bind=True):
        import madronalib_amd as ml
        from madronalib_amd import patches
        from madronalib_amd.sharding import cfg5_voice_params
        self.eng, self.fused, self.N, self.P, self.V = eng, fused, N, cfg["polyphony"], N * cfg["polyphony"]
        self.group, self.mix, self.maxT = group, tuple(mix), max_vectors
        V = self.V
        self.ev = ml.Events(eng, N, self.P, cfg.get("sr", 48000.0))
        self.ev.configure(mpe=0, unison=cfg.get("unison", 0), mod_cc=cfg.get("mod_cc", 16), pitch_bend=cfg.get("bend", 7.0),
                          glide_seconds=cfg.get("glide", 0.0), drift=cfg.get("drift", 0.0))
        self.ev.set_wanted_rows([0, 1])
        desc, outs = patches.synth16(pitch_input=True, event_rows=fused) if patch == "synth" else small_desc(fused)
        listed = switch or not fused             # (a graph with event rows and no switch has no listed form at all)
        g = ml.Graph(eng, V, desc, outs, output_groups={0: group} if group else None, compile_now=False, voice_lists=listed,
                     voice_list_groups=listed and bool(group), voice_list_events=fused and switch)
        for o in self.mix:
            g.set_output_mixdown(o, True)
        g.compile()
        g.clear()
        if patch == "synth":
            params, coeffs, seeds = cfg5_voice_params(0, V, V, ml)
            for k, v in params.items():
                if k != "pitch":
                    g.set_param(k, v if np.ndim(v) else float(v))
            for k, c in coeffs.items():
                g.set_coeffs(k, [np.ascontiguousarray(r) for r in c])
            g.set_state("noise", 0, seeds)
            self.procs = [d["name"] for d in desc if d["type"] == "proc"]
        else:
            g.set_coeffs("lp", [np.full(V, c, np.float32) for c in np.atleast_1d(ml.OnePole.makeCoeffs(0.15))])
            self.procs = ["lp"]
        if fused and bind:
            g.bind_events(self.ev)
        if fused:
            self.ev.reserve_for_graph(max_vectors)
        if listed and group:
            g.reserve_voice_list_groups(V)
        elif listed:
            g.reserve_voice_list(V)
        if self.mix:
            g.reserve_mixdown(max_vectors)
        self.g, self.n_out = g, len(outs)
        self._buffers(max_vectors)

    def _buffers(self, max_vectors):
        n = 4 * self.V * max_vectors * 64
        self.d_out = [self.eng.alloc(n + 64) for _ in range(self.n_out)]
        self.d_peak = self.eng.alloc(4 * self.V + 64)
        self.rows = [self.eng.alloc(n), self.eng.alloc(n)]

    def add_block(self, instruments, b, block=BLOCK):
        import madronalib_amd as ml
        bi, be = [], []
        for i, evs in enumerate(instruments):
            for e in evs:
                if b * block <= e[3] < (b + 1) * block:
                    bi.append(i)
                    be.append(ml.Event(e[0], e[1], e[2], e[3] - b * block, e[4], e[5]))
        self.ev.add_events(bi, be)

    def sounding(self, T, off):
        self.ev.route_ahead(T, off)
        return self.ev.sounding_voices()

    def launch(self, T, off, L):
        """One launch with the list L. Returns (outputs - [rows][64 T] each, a mixed-down one [64 T] -, peaks [K], the comparator's pitch and
        gate rows [V][64 T] or None)."""
        from madronalib_amd.constants import Layout
        g, K = self.g, len(L)
        g.set_voice_list(L)
        self.d_peak.upload(np.full(self.V + 16, 0xABCD1234, np.uint32))
        rows = None
        if self.fused:
            call = g.process_events_listed_groups if self.group else g.process_events_listed
            call(T, off, [], self.d_out, out_layout=Layout.VOICE_MAJOR, d_peak=self.d_peak)
        else:
            self.ev.process(T, off, self.rows + [None] * 6, Layout.VOICE_MAJOR)
            rows = [r.download(np.float32, self.V * T * 64).reshape(self.V, T * 64).copy() for r in self.rows]
            call = g.process_listed_groups if self.group else g.process_listed
            call(T, [self.rows[1] if nm == "gate" else self.rows[0] for nm in g.inputs], self.d_out, in_layout=Layout.VOICE_MAJOR,
                 out_layout=Layout.VOICE_MAJOR, d_peak=self.d_peak)
        outs = []
        for o, d in enumerate(self.d_out):
            if o in self.mix:
                outs.append(d.download(np.float32, 64 * T).copy())
            else:
                r = len(g.listed_groups) if (self.group and o == 0) else K
                outs.append(d.download(np.float32, r * T * 64).reshape(r, T * 64).copy())
        peaks = self.d_peak.download(np.uint32, self.V + 16)
        assert (peaks[K:] == 0xABCD1234).all()          # K words, no more
        return outs, peaks[:K].copy(), rows

    def launch_all(self, T, off):
        """One launch of ALL voices by the unlisted calls: mlgpu_graph_process_events, or the comparator's mlgpu_events_process and
        mlgpu_graph_process of the twin graph. Returns the outputs, [V][64 T] each, a mixed-down one [64 T]."""
        from madronalib_amd.constants import Layout
        g = self.g
        if self.fused:
            g.process_events(T, off, [], self.d_out, out_layout=Layout.VOICE_MAJOR)
        else:
            self.ev.process(T, off, self.rows + [None] * 6, Layout.VOICE_MAJOR)
            g.process(T, [self.rows[1] if nm == "gate" else self.rows[0] for nm in g.inputs], self.d_out, in_layout=Layout.VOICE_MAJOR,
                      out_layout=Layout.VOICE_MAJOR)
        return [d.download(np.float32, 64 * T).copy() if o in self.mix else d.download(np.float32, self.V * T * 64).reshape(self.V, T * 64).copy()
                for o, d in enumerate(self.d_out)]

    def state(self):
        return np.stack([self.g.get_state(p, i) for p in self.procs for i in range(self.g.num_state(p))])

    def close(self):
        self.g.close()
        self.ev.close()


def launches_of(vectors=(3, 3, 2)):
    done = 0
    for T in vectors:
        yield T, done * 64
        done += T


def tails_lists():
    """The list of a launch: sounding_voices() united with the voices that sounded in the two launches before."""
    hist = []

    def make(s):
        L = np.unique(np.concatenate([s] + hist[-2:])).astype(np.uint32) if (len(s) or hist) else np.zeros(0, np.uint32)
        hist.append(s)
        return L
    return make


def run_pair(eng, cfg, instruments, make_list=None, patch="small", group=0, mix=(), vectors=(3, 3, 2), n_blocks=N_BLOCKS, check=None):
    """The fused rig and the comparator through the performance with the same lists; every launch's outputs and peaks compared.
    Returns the per-launch records (L, sounding set, fused outputs, comparator's rows) and the two rigs (the caller closes them)."""
    a, b = Rig(eng, cfg, len(instruments), True, patch, group, mix), Rig(eng, cfg, len(instruments), False, patch, group, mix)
    make_list = make_list or tails_lists()
    log = []
    for blk in range(n_blocks):
        a.add_block(instruments, blk), b.add_block(instruments, blk)
        for T, off in launches_of(vectors):
            s = a.sounding(T, off)
            L = make_list(s)
            ya, pa, _ = a.launch(T, off, L)
            yb, pb, rows = b.launch(T, off, L)
            assert not np.any((rows[0] == 0) & np.signbit(rows[0])), "the comparator's pitch rows hold a -0.0"
            what = f"block {blk} offset {off} K {len(L)}"
            if check is None:
                for o in range(len(ya)):
                    assert_bits_equal(ya[o], yb[o], True, f"{what}: output {o}")
                assert_bits_equal(pa, pb, False, f"{what}: peaks")
            else:
                check(L, ya, yb, pa, pb, what)
            log.append((L, s, ya, rows))
        a.ev.clear_events(), b.ev.clear_events()
    return log, a, b


def performances(name, n=6, n_blocks=N_BLOCKS, drift=0.0):
    cfg = dict(SCENARIOS[name], drift=drift)
    kind = "sustain" if name == "sustain" else "midi"
    return cfg, [performance(kind, 100 * k + len(name), BLOCK * n_blocks, cfg["polyphony"]) for k in range(n)]


@pytest.mark.parametrize("name", ["midi_poly4", "midi_steal2", "unison3", "sustain", "poly1"])
def test_scenarios_with_the_hosts_lists(eng, name):
    """The instrument bank's voice (synth16 with event rows), 6 instruments, launches of 3, 3, 2 vectors, drift 0; the list per launch
    is sounding_voices() and the voices that sounded in the two launches before - K changes all the time and is 0 before the first
    note. Outputs and d_peak against the comparator (see the module's docstring: HIP against HIP, one step from the reference)."""
    cfg, instruments = performances(name)
    # (one block later: the first launches have nobody to list)
    instruments = [[(e[0], e[1], e[2], e[3] + BLOCK, e[4], e[5]) for e in evs if e[3] + BLOCK < BLOCK * N_BLOCKS] for evs in instruments]
    log, a, b = run_pair(eng, cfg, instruments, patch="synth")
    sizes = [len(L) for L, _, _, _ in log]
    assert sizes[0] == 0 and max(sizes) > 0 and len(set(sizes)) >= 2    # (a bank of two-voice instruments soon has every voice sounding)
    assert max(np.abs(y[0]).max() for _, _, y, _ in log if y[0].size) > 0
    a.close(), b.close()


@pytest.mark.parametrize("P", [4, 16])
def test_lane_plan(eng, P):
    """process_events_listed_groups, G = P: the J rows of the instruments' sums and the peaks against the comparator's
    process_listed_groups. Instrument 0 is listed whole, of instrument 2 - which plays nothing - one voice, the others by the host's
    rule: instruments with one, some and all voices listed occur. Every fifth launch has an empty list: the events object advances, no
    voice kernel runs, and the launches after it still equal the comparator's."""
    cfg, instruments = performances("midi_poly4" if P == 4 else "midi_poly16")
    cfg = dict(cfg, bend=7.0)
    instruments[2] = []
    make = tails_lists()
    forced = np.concatenate([np.arange(P), [2 * P + 1]]).astype(np.uint32)
    n = [0]

    def lists(s):
        n[0] += 1
        L = np.union1d(make(s), forced).astype(np.uint32)
        return np.zeros(0, np.uint32) if n[0] % 5 == 0 else L
    log, a, b = run_pair(eng, cfg, instruments, make_list=lists, patch="synth", group=P)
    assert sum(1 for L, _, _, _ in log if L.size == 0) == 4 and log[-1][0].size > 0
    assert max(np.abs(y[0]).max() for _, _, y, _ in log[5:] if y[0].size) > 0
    counts = set()
    for L, _, y, _ in log:
        per = np.bincount(L // P, minlength=6)
        assert y[0].shape[0] == np.count_nonzero(per)
        counts |= set(per.tolist())
    assert 1 in counts and P in counts and any(1 < c < P for c in counts)
    assert_bits_equal(a.state(), b.state(), False, "graph state after listed and empty launches")
    a.close(), b.close()


def test_ragged_and_remapped(eng):
    """801 x 3 = 2 403 voices, every seventh instrument playing; the list is all voices but every ninth: K = 2 136 - nine workgroups,
    eight of them remapped, the last ragged."""
    cfg = dict(polyphony=3, glide=0.01, drift=0.0)
    evs = performance("midi", 11, BLOCK * 2, 3)
    instruments = [evs if k % 7 == 0 else [] for k in range(801)]
    L = np.array([v for v in range(2403) if v % 9 != 8], np.uint32)
    assert len(L) == 2136
    log, a, b = run_pair(eng, cfg, instruments, make_list=lambda s: L, n_blocks=2)
    assert max(np.abs(y[1]).max() for _, _, y, _ in log) > 0
    a.close(), b.close()


@pytest.mark.parametrize("drift", [0.0, 0.5])
def test_mixdown_of_all_voices_with_spare_lanes(eng, drift):
    """V = 120 (40 x 3), K = 65: 63 spare lanes run the list's last voice - its CtlVoice included - again. The mixed-down output, the
    plain ones, the peaks and the last listed voice's graph state against the comparator. With drift 0.5 (the list is constant since
    clear) the words the spare lanes store a second time - the drift glide's words and its moving mCurrVec slots - reach the pitch row:
    the last listed voice's is the comparator's only if those stores are the same words with the same bits."""
    cfg = dict(polyphony=3, glide=0.01, drift=drift)
    instruments = [performance("midi", 300 + k, BLOCK * 3, 3) for k in range(40)]
    L = np.sort(np.random.default_rng(5).choice(120, 65, replace=False)).astype(np.uint32)
    log, a, b = run_pair(eng, cfg, instruments, make_list=lambda s: L, mix=(2,), n_blocks=3)
    assert max(np.abs(y[2]).max() for _, _, y, _ in log) > 0
    sa, sb = a.state(), b.state()
    assert_bits_equal(sa[:, L[-1]], sb[:, L[-1]], False, "the last listed voice's state")
    assert_bits_equal(sa, sb, False, "graph state")
    a.close(), b.close()


def test_the_plain_kernel_with_spare_lanes(eng):
    """With the switch, a graph with event rows and the mixdown of all voices need not be whole wavefronts in its plain kernel either:
    V = 120, mlgpu_graph_process_events of all voices - the 8 spare lanes run voice 119 and its CtlVoice again - against
    mlgpu_events_process + mlgpu_graph_process of the twin graph. Drift 0.5, so the twice-stored glide words reach the pitch row."""
    cfg = dict(polyphony=3, glide=0.01, drift=0.5)
    instruments = [performance("midi", 300 + k, BLOCK * 3, 3) for k in range(40)]
    a, b = Rig(eng, cfg, 40, True, mix=(2,)), Rig(eng, cfg, 40, False, mix=(2,))
    loud = 0.0
    for blk in range(3):
        a.add_block(instruments, blk), b.add_block(instruments, blk)
        for T, off in launches_of():
            ya, yb = a.launch_all(T, off), b.launch_all(T, off)
            for o in range(3):
                assert_bits_equal(ya[o], yb[o], True, f"block {blk} offset {off}: output {o}")
            loud = max(loud, float(np.abs(ya[2]).max()), float(np.abs(ya[0][119]).max()))
        a.ev.clear_events(), b.ev.clear_events()
    assert loud > 0
    assert_bits_equal(a.state(), b.state(), False, "graph state")
    a.close(), b.close()


def test_drift_with_a_constant_list(eng):
    """Drift 0.5, a list constant since clear: the listed voices' drift glides have run in every launch - every output equals."""
    cfg, instruments = performances("midi_poly4", drift=0.5)
    L = np.array([v for v in range(24) if v % 5 != 3], np.uint32)
    log, a, b = run_pair(eng, cfg, instruments, make_list=lambda s: L)
    assert any(np.any(rows[0][:, 1:] != rows[0][:, :-1]) for _, _, _, rows in log)
    a.close(), b.close()


def test_drift_with_changing_lists(eng):
    """Drift 0.5, the host's changing lists: voices listed in every launch equal the comparator in every output and in their peaks; the
    gate-derived output of EVERY listed voice equals it; one launch of 8 vectors equals launches of 3, 3, 2."""
    cfg, instruments = performances("midi_poly4", drift=0.5)
    always = np.array([0, 5, 6, 23], np.uint32)

    def check(L, ya, yb, pa, pb, what):
        assert_bits_equal(ya[1], yb[1], True, f"{what}: the gate-derived output of every listed voice")
        at = np.searchsorted(L, always)
        for o in (0, 2):
            assert_bits_equal(ya[o][at], yb[o][at], True, f"{what}: output {o} of the voices listed in every launch")
        assert_bits_equal(pa[at], pb[at], False, f"{what}: peaks of the voices listed in every launch")

    def lists():
        make = tails_lists()
        return lambda s: np.union1d(make(s), always).astype(np.uint32)
    log3, a, b = run_pair(eng, cfg, instruments, make_list=lists(), check=check)
    a.close(), b.close()
    # the same lists per block (a block's list: the union of its three launches'), one launch of 8 against 3, 3, 2
    block_lists = [np.unique(np.concatenate([log3[3 * k + j][0] for j in range(3)])).astype(np.uint32) for k in range(N_BLOCKS)]
    runs = []
    for vectors in ((8,), (3, 3, 2)):
        r = Rig(eng, cfg, 6, True)
        chunks = []
        for blk in range(N_BLOCKS):
            r.add_block(instruments, blk)
            ys = []
            for T, off in launches_of(vectors):
                r.ev.route_ahead(T, off)
                ys.append(r.launch(T, off, block_lists[blk])[0])
            chunks.append([np.concatenate([y[o] for y in ys], 1) for o in range(3)])
            r.ev.clear_events()
        runs.append(chunks)
        r.close()
    for blk in range(N_BLOCKS):
        for o in range(3):
            assert_bits_equal(runs[1][blk][o], runs[0][blk][o], True, f"block {blk} output {o}: launches of 3, 3, 2 against one of 8")


def test_handover_to_the_unlisted_form(eng):
    """Drift 0: four listed blocks (the list: every voice that has sounded so far - an unlisted voice of this graph has a gate of zero
    and a state of zeros, which running it would leave as they are), then four blocks of mlgpu_graph_process_events on the same
    objects: equal to a run that never used lists."""
    from madronalib_amd.constants import Layout
    cfg, instruments = performances("midi_poly4")
    outs = []
    for listed_blocks in (4, 0):
        r = Rig(eng, cfg, 6, True)
        ever = np.zeros(0, np.uint32)
        chunks = []
        for blk in range(N_BLOCKS):
            r.add_block(instruments, blk)
            for T, off in launches_of():
                if blk < listed_blocks:
                    ever = np.union1d(ever, r.sounding(T, off)).astype(np.uint32)
                    y = r.launch(T, off, ever)[0]
                    full = [np.zeros((r.V, 64 * T), np.float32) for _ in range(3)]
                    for o in range(3):
                        full[o][ever] = y[o]
                else:
                    r.g.process_events(T, off, [], r.d_out, out_layout=Layout.VOICE_MAJOR)
                    full = [d.download(np.float32, r.V * T * 64).reshape(r.V, T * 64).copy() for d in r.d_out]
                chunks.append(full)
            r.ev.clear_events()
        outs.append(chunks)
        r.close()
    for k, (got, want) in enumerate(zip(*outs)):
        if k < 12:      # the listed blocks: the listed voices' rows - where the listed run has none, the plain run's `lp` is silent
            assert_bits_equal(got[1], want[1], True, f"launch {k}: the gate-derived output (listed blocks)")
            continue
        for o in range(3):
            assert_bits_equal(got[o], want[o], True, f"launch {k}: output {o} (after the handover)")
    assert max(np.abs(c[1]).max() for c in outs[0][12:]) > 0


def test_unlisted_voices_are_not_touched_and_an_empty_list_advances_the_events(eng):
    """Unlisted voices' graph state words are unchanged bits across listed launches; a launch with an empty list launches no voice
    kernel and still advances the events object - the next full launch equals the comparator's."""
    cfg, instruments = performances("midi_poly4")
    V = 24
    L = np.array([1, 2, 3, 8, 13, 21], np.uint32)
    unlisted = np.setdiff1d(np.arange(V), L)
    a, b = Rig(eng, cfg, 6, True, "synth"), Rig(eng, cfg, 6, False, "synth")
    phases = np.random.default_rng(9).integers(0, 2 ** 32, V, dtype=np.uint64).astype(np.uint32)
    for r in (a, b):        # state words nothing of a clear would leave
        r.g.set_state("saw", 0, phases)
        r.g.set_state("lp", 0, np.linspace(0.01, 0.2, V).astype(np.float32).view(np.uint32))
    before = a.state()
    everyone = np.arange(V, dtype=np.uint32)
    for blk in range(4):
        a.add_block(instruments, blk), b.add_block(instruments, blk)
        for i, (T, off) in enumerate(launches_of()):
            Lk = [L, np.zeros(0, np.uint32), everyone][i] if blk >= 2 else L
            a.ev.route_ahead(T, off)
            ya, pa, _ = a.launch(T, off, Lk)
            yb, pb, _ = b.launch(T, off, Lk)
            assert_bits_equal(ya[0], yb[0], True, f"block {blk} launch {i}")
            assert_bits_equal(pa, pb, False, f"block {blk} launch {i}: peaks")
            if blk < 2:
                assert_bits_equal(a.state()[:, unlisted], before[:, unlisted], False, "unlisted voices' state words")
        a.ev.clear_events(), b.ev.clear_events()
    assert not np.array_equal(a.state()[:, L], before[:, L])
    assert_bits_equal(a.state(), b.state(), False, "graph state after listed, empty and full launches")
    a.close(), b.close()


@pytest.mark.parametrize("name", ["midi_steal2", "sustain"])
def test_sounding_voices_cover_every_gate(eng, name):
    """Over a whole performance: every voice with a non-zero gate sample in a launch is in that launch's sounding_voices(), and every
    voice in it has a non-zero gate at the launch's last frame or a record in the launch - seen from here: an event of its instrument in
    the launch, or the instrument's awake records, which go out with the first launch of the block that holds its first event."""
    cfg, instruments = performances(name)
    log, a, b = run_pair(eng, cfg, instruments, make_list=lambda s: s.astype(np.uint32))
    P = cfg["polyphony"]
    k = 0
    for blk in range(N_BLOCKS):
        for T, off in launches_of():
            L, s, _, rows = log[k]
            k += 1
            gate = rows[1]
            assert np.all(np.isin(np.flatnonzero(np.any(gate != 0, axis=1)), s)), f"block {blk} offset {off}: a sounding voice is missing"
            lo, hi = blk * BLOCK + off, blk * BLOCK + off + 64 * T
            has_events = {i for i, evs in enumerate(instruments) if any(lo <= e[3] < hi for e in evs)}
            wakes = {i for i, evs in enumerate(instruments) if off == 0 and evs and blk * BLOCK <= min(e[3] for e in evs) < (blk + 1) * BLOCK}
            for v in s:
                assert gate[v, -1] != 0 or (v // P) in has_events or (v // P) in wakes, f"block {blk} offset {off}: voice {v} neither sounds nor has a record"
    assert max(len(s) for _, s, _, _ in log) > 1 and min(len(s) for _, s, _, _ in log) < max(len(s) for _, s, _, _ in log)
    a.close(), b.close()


def test_refusals_leave_everything_untouched(eng):
    """No switch; an MPE object; nothing bound; a route_ahead mismatch; a too-small capacity. Each leaves the outputs (guard words), the
    graph's state and the pending events as they were: the next valid call gives the comparator's bits."""
    import ctypes

    import madronalib_amd as ml
    from madronalib_amd.constants import Layout, Status
    cfg, instruments = performances("midi_poly4")
    V = 24
    L = np.arange(0, V, 1, dtype=np.uint32)[np.arange(V) % 4 != 2]

    def refused(status, words, fn, *args, **kw):
        with pytest.raises(ml.MlgpuError) as ei:
            fn(*args, **kw)
        assert ei.value.status == status and all(w in str(ei.value) for w in words), str(ei.value)
    guard = np.full(V * 8 * 64 + 16, 7.5, np.float32)

    def untouched(r, state):
        for d in r.d_out:
            assert np.array_equal(d.download(np.float32, guard.size), guard)
        assert_bits_equal(r.state(), state, False, "graph state after the refusal")

    def armed(r):
        for d in r.d_out:
            d.upload(guard)
        return r.state()
    # a graph with event rows made without the switch: refused; the next valid call - it has no listed one - is the comparator's
    r, c = Rig(eng, cfg, 6, True, switch=False), Rig(eng, cfg, 6, False)
    r.add_block(instruments, 0), c.add_block(instruments, 0)
    state = armed(r)
    for call in (r.g.process_events_listed, r.g.process_events_listed_groups):
        refused(Status.ERR_INVALID, ["mlgpu_graph_enable_voice_list_events"], call, 8, 0, [], r.d_out, d_peak=r.d_peak)
    untouched(r, state)
    for o, (y, want) in enumerate(zip(r.launch_all(8, 0), c.launch_all(8, 0))):
        assert_bits_equal(y, want, True, f"no switch: output {o} of the next valid call")
    assert np.abs(want).max() > 0
    r.close(), c.close()
    # nothing bound: refused; bound, the same call gives the comparator's bits
    r, c = Rig(eng, cfg, 6, True, bind=False), Rig(eng, cfg, 6, False)
    r.add_block(instruments, 0), c.add_block(instruments, 0)
    r.g.set_voice_list(L)
    state = armed(r)
    refused(Status.ERR_INVALID, ["graph_bind_events"], r.g.process_events_listed, 8, 0, [], r.d_out, d_peak=r.d_peak)
    untouched(r, state)
    r.g.bind_events(r.ev)
    (ya, pa, _), (yb, pb, _) = r.launch(8, 0, L), c.launch(8, 0, L)
    for o in range(3):
        assert_bits_equal(ya[o], yb[o], True, f"nothing bound: output {o} of the next valid call")
    assert_bits_equal(pa, pb, False, "nothing bound: peaks of the next valid call")
    r.close(), c.close()
    # an object switched to MPE after it was bound: refused; the block's events are still there - mlgpu_events_process, the call an MPE
    # object has, gives the rows of a twin MPE object with the same events
    r, c = Rig(eng, cfg, 6, True), Rig(eng, cfg, 6, False)
    r.ev.configure(mpe=1), c.ev.configure(mpe=1)
    r.add_block(instruments, 0), c.add_block(instruments, 0)
    r.g.set_voice_list(L)
    state = armed(r)
    refused(Status.ERR_UNSUPPORTED, ["MIDI"], r.g.process_events_listed, 8, 0, [], r.d_out, d_peak=r.d_peak)
    refused(Status.ERR_UNSUPPORTED, ["MIDI"], r.ev.sounding_voices)
    untouched(r, state)
    for x in (r, c):
        x.ev.process(8, 0, x.rows + [None] * 6, Layout.VOICE_MAJOR)
    for k in range(2):
        got, want = (x.rows[k].download(np.float32, V * 8 * 64) for x in (r, c))
        assert_bits_equal(got, want, True, f"MPE: row {k} of the next valid call")
    assert np.abs(want).max() > 0
    r.close(), c.close()
    a, b = Rig(eng, cfg, 6, True), Rig(eng, cfg, 6, False)
    for blk in range(3):
        a.add_block(instruments, blk), b.add_block(instruments, blk)
        for T, off in launches_of():
            a.g.set_voice_list(L)
            for d in a.d_out:
                d.upload(guard)
            state = a.state()
            refused(Status.ERR_RANGE, ["mlgpu_events_reserve_for_graph"], a.g.process_events_listed, 9, off, [], a.d_out, out_layout=Layout.VOICE_MAJOR, d_peak=a.d_peak)
            refused(Status.ERR_RANGE, ["mlgpu_events_reserve_for_graph"], a.ev.route_ahead, 9, off)
            s = a.sounding(T, off)
            args = ([], a.d_out)
            kw = dict(out_layout=Layout.VOICE_MAJOR, d_peak=a.d_peak)
            # other values than the routed launch's; events and a second route_ahead while it is pending
            refused(Status.ERR_INVALID, ["mlgpu_events_route_ahead"], a.g.process_events_listed, T + 1, off, *args, **kw)
            refused(Status.ERR_INVALID, ["mlgpu_events_route_ahead"], a.g.process_events_listed, T, off + 64, *args, **kw)
            refused(Status.ERR_INVALID, [], a.g.process_events, T, off + 64, *args, out_layout=Layout.VOICE_MAJOR)
            refused(Status.ERR_INVALID, ["mlgpu_events_route_ahead"], a.ev.route_ahead, T, off)
            refused(Status.ERR_INVALID, ["mlgpu_events_route_ahead"], a.ev.add_event, 0, ml.Event(1, 1, 60, 0, 0.0, 0.5))
            refused(Status.ERR_INVALID, ["negative"], a.g.process_events_listed, T, -1, *args, **kw)
            refused(Status.ERR_INVALID, ["misaligned peaks"], a.g.process_events_listed, T, off, *args, out_layout=Layout.VOICE_MAJOR, d_peak=a.d_peak.ptr + 2)
            refused(Status.ERR_INVALID, ["lane plan"], a.g.process_events_listed_groups, T, off, *args, **kw)
            # a capacity too small for the set: its size comes back
            n = ctypes.c_size_t(99)
            small = np.zeros(max(1, len(s)), np.uint32)
            st = a.ev.L.mlgpu_events_sounding_voices(a.ev.h, small.ctypes.data_as(ctypes.c_void_p), max(0, len(s) - 1), ctypes.byref(n))
            assert (st == Status.ERR_RANGE and n.value == len(s)) if len(s) else st == Status.OK
            for d in a.d_out:
                assert np.array_equal(d.download(np.float32, guard.size), guard)
            assert_bits_equal(a.state(), state, False, "graph state after the refusals")
            assert np.array_equal(a.ev.sounding_voices(), s)
            ya, pa, _ = a.launch(T, off, L)
            yb, pb, _ = b.launch(T, off, L)
            for o in range(3):
                assert_bits_equal(ya[o], yb[o], True, f"block {blk} offset {off}: output {o} after the refusals")
            assert_bits_equal(pa, pb, False, "peaks after the refusals")
        a.ev.clear_events(), b.ev.clear_events()
    a.close(), b.close()
