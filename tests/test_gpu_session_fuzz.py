"""Session fuzz on the device: seeded random sessions of a live voice bank (session_steps) - voice lists, listed and plain launches, update
records, steals, voice moves between two objects, refused calls - walked through the library and through the host model (session_model)
side by side. The model is the project's CPU oracle on the gathered voices with per-voice ring memory, so graphs with delay rings are
compared with an independent reference too, in ring layouts 0, 1 and 4 (and 2, which has no listed form, in sessions without lists).

One session: every call goes out back to back on the engine's stream, each launch into guarded device buffers of its own that were made
and filled before the first call; nothing is downloaded and nothing waits until the last step (every second seed waits and compares after
each step instead, so that a failure can be placed). Then every launch's outputs, mixed-down rows and peaks against the model, bit for
bit, and the guard words; every params, coefficient and state row through the getters; one exported record per voice of a sample of
voices, its table words in the documented order. The session's last steps are a drain: every delay time at ring length - 64 and all voices
for ring length / 64 + 1 DSPVectors, so that what is left in the rings comes out.

A longer campaign (seeds per family and ring layout; MLGPU_SESSION_FAMILIES=bank,synth narrows it):
MLGPU_SESSION_FIRST=1000 MLGPU_SESSION_SEEDS=80 python -m pytest tests/test_gpu_session_fuzz.py -m gpu"""
import os

import numpy as np
import pytest

import session_steps as ss
import tails_rule
from inputs import assert_bits_equal
from madronalib_amd.constants import Layout, Status, UpdateTarget

GUARD = np.uint32(0x7FC5A5A5)   # what the memory behind an output holds before a launch
TARGETS = {"param": UpdateTarget.PARAM, "coeff": UpdateTarget.COEFF, "state": UpdateTarget.STATE, "input_const": UpdateTarget.INPUT_CONST,
           "clear": UpdateTarget.CLEAR, "clear_rings": UpdateTarget.CLEAR_RINGS}
FIRST, SEEDS = int(os.environ.get("MLGPU_SESSION_FIRST", "0")), int(os.environ.get("MLGPU_SESSION_SEEDS", "0")) or None
FAMILIES = tuple(f for f in os.environ.get("MLGPU_SESSION_FAMILIES", "").split(",") if f) or ss.FAMILIES
CASES = ss.default_cases(FIRST, SEEDS, FAMILIES)
_engines = {}


@pytest.fixture(scope="module")
def engines():
    """parts -> an engine with that set_launch_parts (1: always one launch; 2: a plain launch of more than 2 048 voices in two parts)."""
    import madronalib_amd as ml
    for parts in (1, 2):
        _engines[parts] = ml.Engine(0)
        _engines[parts].set_launch_parts(parts)
    yield _engines
    for e in _engines.values():
        e.close()
    _engines.clear()


# ---- the objects ------------------------------------------------------------------------------------------------------------------------------
def make_object(eng, session, o, layout):
    import madronalib_amd as ml
    f, V, t = session.family, session.shapes[o], session.tables[o]
    if f == "bank":
        b = eng.bank(ss.BANK_PROCS, V)
        b.clear()
        b.set_all_coeffs(t["coeffs"])
        b.set_all_state(t["state"])
        b.set_input_const(t["in_const"])
        b.reserve_voice_list(V)
        obj = b
    else:
        desc, outputs, mix, _ = ss.description(f)
        rings = f != "synth"
        g = ml.Graph(eng, V, desc, outputs, delay_windows=layout if rings else False, compile_now=False, voice_lists=session.lists,
                     voice_list_rings=session.lists and rings and layout in (1, 4))
        for out in mix:
            g.set_output_mixdown(out, True)
        g.compile()
        assert not rings or g.delay_layout == layout, f"asked for ring layout {layout}, the compile resolved to {g.delay_layout}"
        if mix:
            g.reserve_mixdown(ss.RING // 64 + 1)
        g.clear()
        for name, p in t["params"].items():
            g.set_param(name, p)
        for name, co in t["coeffs"].items():
            for i in range(co.shape[0]):
                g.set_coeff(name, i, np.ascontiguousarray(co[i]))
        for name, st in t["states"].items():
            for i in range(st.shape[0]):
                g.set_state(name, i, st[i])
        if session.lists:
            g.reserve_voice_list(V)
        obj = g
    obj.reserve_updates(4096)
    obj.reserve_voice_records(16)
    return obj


def updates(obj, records, bank):
    import madronalib_amd as ml
    return [ml.Update(int(node) if bank or node == -1 else obj.ids[node], TARGETS[target], index, first, n, bits) for target, node, index, first, n, bits in records]


class Buffers:
    """Device buffers of one session, freed together."""

    def __init__(self, eng):
        self.eng, self.all = eng, []

    def alloc(self, nbytes):
        self.all.append(self.eng.alloc(max(16, nbytes)))
        return self.all[-1]

    def guarded(self, words, guard_words):
        d = self.alloc(4 * (words + guard_words))
        d.upload(np.full(words + guard_words, GUARD, np.uint32))
        return d

    def rows(self, rows, layout, vectors):
        """[R][64 vectors] numpy -> a device signal of R rows in `layout`."""
        rows = np.ascontiguousarray(rows, np.float32)
        d = self.alloc(rows.nbytes)
        d.upload(rows)
        if layout == Layout.VOICE_MAJOR:
            return d
        d2 = self.alloc(rows.nbytes)
        self.eng.layout_convert(d, Layout.VOICE_MAJOR, d2, layout, rows.shape[0], vectors)
        return d2

    def free(self):
        for d in self.all:
            d.free()
        self.all = []


def prepare_launch(bufs, session, st, e, V, io, n_outputs, mix):
    """Everything a launch reads and writes, made before the session's first call."""
    f, n, K = session.family, st["n"], e["L"].size
    p = dict(K=K, d_in=[], d_ctl=[], d_gains=None)
    if f != "bank":
        inputs, controls = ss.launch_signals(f, V, n, st["sig"], st.get("drain", False))
        p["d_in"] = [bufs.rows(a, io, n) for a in inputs.values()]
        p["d_ctl"] = [bufs.rows(np.ascontiguousarray(a.T), Layout.VOICE_MAJOR, n) for a in controls.values()]
    elif st.get("mixdown"):
        p["d_gains"] = bufs.alloc(4 * V)
        p["d_gains"].upload(ss.launch_gains(V, st["gains"]))
    p["rows"] = [1 if (o in mix or st.get("mixdown")) else K for o in range(n_outputs)]
    p["d_out"] = [bufs.guarded(r * 64 * n, 64 * n) for r in p["rows"]]
    p["d_peak"] = bufs.guarded(K, 1)
    return p


def check_launch(bufs, session, st, e, p, io, what):
    n, K, eng = st["n"], p["K"], bufs.eng
    for o, (d, r) in enumerate(zip(p["d_out"], p["rows"])):
        raw = d.download(np.uint32)
        assert (raw[r * 64 * n:] == GUARD).all(), f"{what}: the row behind output {o} was written"
        if o in e["mix"]:
            got, want = raw[:64 * n].view(np.float32), e["mix"][o]
        elif K == 0 or io == Layout.VOICE_MAJOR:
            got, want = raw[:K * 64 * n].view(np.float32).reshape(K, 64 * n), e["ys"][o]
        else:
            d_vm = bufs.alloc(4 * K * 64 * n)
            eng.layout_convert(d, io, d_vm, Layout.VOICE_MAJOR, K, n)
            got, want = d_vm.download(np.float32, K * 64 * n).reshape(K, 64 * n), e["ys"][o]
        assert_bits_equal(got, want, True, f"{what}: output {o} ({'mixed down' if o in e['mix'] else f'{K} rows'}) against the model")
    pk = p["d_peak"].download(np.uint32)
    if p.get("peaks_written", True):
        assert_bits_equal(pk[:K], e["peaks"], False, f"{what}: peaks against the model")
        assert pk[K] == GUARD, f"{what}: the word behind d_peak[K] was written"
    else:
        assert (pk == GUARD).all(), f"{what}: a plain launch wrote d_peak"


def read_tables(obj, world, bank):
    t = {}
    for key in world.tables():
        kind, node, i = key
        if kind == "param":
            t[key] = obj.get_param(node).view(np.uint32)
        elif kind == "coeff":
            t[key] = obj.get_coeff(node, i).view(np.uint32)
        elif kind == "state":
            t[key] = obj.get_state(node, i).view(np.uint32)
        else:
            t[key] = obj.get_input_const().view(np.uint32)
    return t


# ---- one session ------------------------------------------------------------------------------------------------------------------------------
def run_session(eng, session, layout, step_sync, steps=None):
    """The session on the device against the model. steps: a reduced step list instead of the session's own."""
    import madronalib_amd as ml
    if steps is not None:
        session = type(session)(**{**vars(session), "steps": steps})
    f, bank = session.family, session.family == "bank"
    what0 = f"{f} layout {layout} seed {session.seed}"
    worlds, launches = ss.walk_model(session)
    by_step = {e["step"]: e for e in launches}
    io = Layout.QUAD if session.seed % 4 < 2 else Layout.VOICE_MAJOR
    listed_for_plain = f == "pitchbend" and layout == 4      # the plain call is refused there after a listed launch or an import
    n_outputs, mix = (1, ()) if bank else (len(ss.description(f)[1]), ss.description(f)[2])
    bufs = Buffers(eng)
    objs = {o: make_object(eng, session, o, layout) for o in session.shapes}
    try:
        if bank:
            eng.mixdown_reserve(max(session.shapes.values()), ss.RING // 64 + 1)
        sigs = {o: g.voice_record_signature for o, g in objs.items()}
        W = objs["A"].voice_record_words
        assert sigs["A"] == sigs["B"] != 0 and W == objs["B"].voice_record_words and W % 4 == 0
        prep = {i: prepare_launch(bufs, session, st, by_step[i], session.shapes[st["obj"]], io, n_outputs, mix) for i, st in enumerate(session.steps) if i in by_step}
        slots = {st["slot"]: bufs.alloc(4 * W * len(st["voices"])) for st in session.steps if st["kind"] == "move" and st["op"] == "export"}
        scratch = bufs.alloc(4 * W * 4)
        cur = {o: np.zeros(0, np.uint32) for o in objs}
        eng.sync()
        for i, st in enumerate(session.steps):
            g, kind, what = objs[st["obj"]], st["kind"], f"{what0} step {i} ({st['kind']} on {st['obj']})"
            if kind == "list":
                g.set_voice_list(st["L"])
                cur[st["obj"]] = st["L"]
                assert g.voice_list_size == st["L"].size
            elif kind in ("listed", "plain"):
                p, n = prep[i], st["n"]
                as_listed = kind == "listed" or listed_for_plain
                if kind == "plain" and listed_for_plain:
                    g.set_voice_list(np.arange(g.V, dtype=np.uint32))
                p["peaks_written"] = as_listed
                if bank and kind == "plain":
                    g.process(n, p["d_out"][0], io)
                elif bank and st["mixdown"]:
                    g.process_listed_mixdown(n, p["d_out"][0], d_gains=p["d_gains"], d_peak=p["d_peak"])
                elif bank:
                    g.process_listed(n, p["d_out"][0], io, d_peak=p["d_peak"])
                elif as_listed:
                    g.process_listed(n, p["d_in"], p["d_out"], io, io, p["d_ctl"], p["d_peak"])
                else:
                    g.process(n, p["d_in"], p["d_out"], io, io, p["d_ctl"])
                if kind == "plain" and listed_for_plain:
                    g.set_voice_list(cur[st["obj"]])
            elif kind in ("updates", "steal"):
                g.apply_updates(updates(g, st["records"], bank))
                if kind == "steal" and st["L"] is not None:
                    g.set_voice_list(st["L"])
                    cur[st["obj"]] = st["L"]
            elif kind == "move" and st["op"] == "export":
                g.export_voices(st["voices"], slots[st["slot"]])
            elif kind == "move":
                g.import_voices(sigs[st["obj"]], st["voices"], slots[st["slot"]])
            elif kind == "refused":
                call, arg = st["call"]
                with pytest.raises(ml.MlgpuError) as ei:
                    if call == "list":
                        g.set_voice_list(np.array(arg, np.uint32))
                    elif call == "updates":
                        g.apply_updates(updates(g, arg, bank))
                    elif call == "export":
                        g.export_voices(np.array(arg, np.uint32), scratch)
                    else:
                        g.import_voices(sigs[st["obj"]] ^ (1 if call == "import_foreign" else 0), np.array(arg, np.uint32), scratch)
                assert ei.value.status == getattr(Status, st["status"]), f"{what}: {call} {arg}: {ei.value}"
                if call == "list":
                    assert g.voice_list_size == cur[st["obj"]].size, f"{what}: a refused list changed the list's length"
            if step_sync and i in by_step:
                eng.sync()
                check_launch(bufs, session, st, by_step[i], prep[i], io, what)
        eng.sync()
        if not step_sync:
            for i, e in by_step.items():
                check_launch(bufs, session, session.steps[i], e, prep[i], io, f"{what0} step {i} ({session.steps[i]['kind']} on {session.steps[i]['obj']})")
        for o, g in objs.items():
            w = worlds[o]
            want, got = w.tables(), read_tables(g, w, bank)
            for key in want:
                assert_bits_equal(got[key], want[key], False, f"{what0}: object {o} row {key} through the getter against the model")
            sample = np.unique(np.array([0, 1, 63, 64, 255, 256, 511, 512, g.V - 2, g.V - 1], np.int64) % g.V).astype(np.uint32)
            rec = g.export_voices(sample, bufs.guarded(W * sample.size, 0)).download(np.uint32, W * sample.size).reshape(sample.size, W)
            for k, v in enumerate(sample):
                words = w.record_table_words(int(v))
                pad = -len(words) % 4
                assert_bits_equal(rec[k, :len(words)], words, False, f"{what0}: object {o} voice {v}: the table words of its record")
                assert (rec[k, len(words):len(words) + pad] == 0).all(), f"{what0}: object {o} voice {v}: the words up to a multiple of 4 are zeros"
                assert (f in ("bank", "synth")) == (len(words) + pad == W), "without rings a record is its table words; with rings it goes on with them"
    finally:
        bufs.free()
        for g in objs.values():
            g.close()


def case_id(c):
    return f"{c[0]}-layout{c[1]}-seed{c[2]}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_session(engines, case):
    """Every second seed waits and compares after each step; every second pair of a bank's seeds runs on an engine that sends a plain launch
    of the 2 352 voices out in two parts on two streams, joined lazily before whatever follows."""
    family, layout, seed, lists = case
    session = ss.make_session(seed, family, lists)
    eng = engines[2 if family == "bank" and (seed // 2) % 2 else 1]
    splits = eng.launch_stats()[0] if family == "bank" else 0
    run_session(eng, session, layout, step_sync=seed % 2 == 1)
    if family == "bank" and eng is engines[2]:
        assert eng.launch_stats()[0] > splits, "no plain launch of this session went out in parts"


# ---- reduced sessions of what the fuzz found ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_regression_a_record_has_zeros_up_to_a_multiple_of_4(engines):
    """Found by synth seed 2: the synth's record is 9 table words and 3 more up to a multiple of 4, which export left as the buffer had
    them - leftovers of an earlier launch's output there - where include/mlgpu.h says zeros. The reduced session: no step at all, and
    the export at its end into a buffer that holds the guard pattern."""
    session = ss.make_session(2, "synth")
    run_session(engines[1], session, 0, step_sync=False, steps=[])


# ---- lists made by the engine: voice tails ---------------------------------------------------------------------------------------------------
QUIET, HOLD, BLOCKS = 1e-4, 2, 14


def tails_blocks(family, V, seed):
    """[(must, records, n)]: per block the voices struck now - cleared and retuned so that they sound and then die away within a few
    DSPVectors -, the update records that do it, and the block's DSPVectors. A bank voice is struck with a frequency and let go in the
    next block with one below 2^-64: it stands still, and a constant dies away in the Bandpass. A string is struck with a short, lossy loop
    and gets input in the block of the strike only."""
    rng = np.random.default_rng([seed, V, 4242])
    blocks, last = [], np.zeros(0, np.int64)
    for b in range(BLOCKS):
        must = np.sort(rng.choice(V, int(rng.integers(0, 24)), replace=False)) if b % 5 != 4 else np.zeros(0, np.int64)
        if b == 2:
            must = np.union1d(must, np.arange(250, 262))       # a run across a 256-voice block's border
        recs = []
        if family == "bank":
            recs += [("input_const", 0, 0, int(v), 1, ss._f32(1e-30)) for v in np.setdiff1d(last, must)]
            for v in must:
                recs += [("clear", -1, 0, int(v), 1, 0), ("input_const", 0, 0, int(v), 1, ss._f32(rng.uniform(0.002, 0.04)))]
        else:
            for v in must:
                recs += [("clear_rings", -1, 0, int(v), 1, 0), ("param", "dt", 0, int(v), 1, ss._f32(rng.uniform(1.0, 30.0))), ("param", "g", 0, int(v), 1, ss._f32(rng.uniform(0.1, 0.3)))]
        blocks.append((must.astype(np.uint32), recs, int(rng.integers(1, 4))))
        last = must
    return blocks


def tails_inputs(family, V, n, must, sig):
    if family == "bank":
        return {}
    x = np.zeros((V, 64 * n), np.float32)
    x[must] = ss.launch_signals(family, V, n, sig)[0]["x"][must]
    return {"x": x}


@pytest.mark.gpu
@pytest.mark.parametrize("family,layout", [("bank", 0), ("string", 0), ("string", 1), ("string", 4)])
def test_session_with_lists_from_voice_tails(engines, family, layout):
    """The lists come from VoiceTails.next_list(must), the engine synchronised before each call; they must be tails_rule.Rule's fed with the
    MODEL's peaks - a device peak that is off by a bit around the threshold, or a list that is, shows here -, and every launch's outputs
    and peaks must be the model's as in the sessions above."""
    import types
    import madronalib_amd as ml
    eng, seed = engines[1], FIRST
    VA = ss.shapes(family)[0]
    session = types.SimpleNamespace(family=family, seed=seed, lists=True, shapes={"A": VA}, tables={"A": ss.initial_tables(family, VA, seed)}, steps=[])
    world = ss.new_world(family, VA, session.tables["A"])
    bank = family == "bank"
    if not bank:      # no string sounds before it is struck
        world.apply([("param", "g", 0, 0, VA, ss._f32(0.0))])
    blocks = tails_blocks(family, VA, seed)
    bufs = Buffers(eng)
    g = make_object(eng, session, "A", layout)
    tails = ml.VoiceTails(eng, VA, VA, depth=4)
    try:
        tails.set_threshold(QUIET, HOLD)
        rule = tails_rule.Rule(hold=HOLD)
        if not bank:
            g.apply_updates(updates(g, [("param", "g", 0, 0, VA, ss._f32(0.0))], bank))
        quiet_bits = int(np.float32(QUIET).view(np.uint32))
        launches, sizes = [], []
        for b, (must, recs, n) in enumerate(blocks):
            what = f"{family} layout {layout} seed {seed} block {b}"
            if recs:
                world.apply(recs)
                g.apply_updates(updates(g, recs, bank))
            eng.sync()
            L, want = tails.next_list(must), rule.next_list(must)
            assert np.array_equal(L, want), f"{what}: the engine's list against the rule on the model's peaks: {np.setxor1d(L, want)[:8]}"
            g.set_voice_list(L)
            inputs = tails_inputs(family, VA, n, must.astype(np.int64), seed * 100 + b)
            if bank:
                y, _, peaks = world.run(L, n)
                e = dict(L=L, n=n, ys=[y], mix={}, peaks=peaks)
            else:
                ys, mix, peaks = world.run(L, n, inputs)
                e = dict(L=L, n=n, ys=ys, mix=mix, peaks=peaks)
            p = dict(K=L.size, d_in=[bufs.rows(a, Layout.QUAD, n) for a in inputs.values()], rows=[L.size], d_out=[bufs.guarded(L.size * 64 * n, 64 * n)], d_peak=bufs.guarded(L.size, 1))
            if bank:
                g.process_listed(n, p["d_out"][0], Layout.QUAD, d_peak=p["d_peak"])
            else:
                g.process_listed(n, p["d_in"], p["d_out"], Layout.QUAD, Layout.QUAD, (), p["d_peak"])
            tails.note(n, p["d_peak"])
            rule.note(n, tails_rule.loud_bits(peaks, quiet_bits))
            launches.append((dict(n=n), e, p, what))
            sizes.append(L.size)
        eng.sync()
        for st, e, p, what in launches:
            check_launch(bufs, session, st, e, p, Layout.QUAD, what)
        # the lists did what the variant is for: voices came, stayed while they sounded, and left
        assert max(sizes) > 20 and any(b < a for a, b in zip(sizes, sizes[1:])), sizes
    finally:
        tails.close()
        bufs.free()
        g.close()
