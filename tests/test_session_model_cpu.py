"""The host model of a session (session_model) and the seeded generator (session_steps), on the CPU alone: what
tests/test_gpu_session_fuzz.py compares the device with must itself be right, and the default sessions must reach what they are for.

Separability: the model gathers the listed voices, runs the oracle on K voices and scatters the state back; V independent one-voice
models that are driven only when their voice is listed must give the same bits - outputs, peaks, every table word, ring and feedback
memory. Update semantics: CLEAR_RINGS(-1) against a fresh world; the later record wins. Coverage and liveness of the default seeds are
conditions on the model's own values, so no kernel can meet them on the model's behalf."""
import numpy as np
import pytest

import session_steps as ss
from inputs import assert_bits_equal
from session_model import CLEAR_RINGS, COEFF, PARAM, STATE, cleared_words
from madronalib_amd.constants import Proc


def family_sessions(family):
    return [ss.make_session(seed, f, lists) for f, _, seed, lists in ss.default_cases(families=(family,))]


# ---- separability ---------------------------------------------------------------------------------------------------------------------------
def one_voice_tables(family, tables, v):
    if family == "bank":
        return dict(coeffs=tables["coeffs"][:, v:v + 1], in_const=tables["in_const"][v:v + 1], state=tables["state"][:, v:v + 1])
    return dict(params={k: a[v:v + 1] for k, a in tables["params"].items()}, coeffs={k: a[:, v:v + 1] for k, a in tables["coeffs"].items()},
                states={k: a[:, v:v + 1] for k, a in tables["states"].items()})


@pytest.mark.parametrize("family", ss.FAMILIES)
def test_the_model_is_v_one_voice_models(family):
    """The first default session of the family every launch's rows and
    peaks, then every per-voice word of both worlds, against one-voice worlds that run only when their voice is listed."""
    f, _, seed, lists = ss.default_cases(families=(family,))[0]
    session = ss.make_session(seed, f, lists)
    singles = {(o, v): ss.new_world(f, 1, one_voice_tables(f, session.tables[o], v)) for o, V in session.shapes.items() for v in range(V)}
    _, launches = ss.walk_model(session)
    by_step = {e["step"]: e for e in launches}
    cur = {o: np.zeros(0, np.uint32) for o in session.shapes}
    slots = {}
    for i, st in enumerate(session.steps):
        o = st["obj"]
        V = session.shapes[o]
        if st["kind"] == "list":
            cur[o] = st["L"]
        elif st["kind"] in ("listed", "plain"):
            e = by_step[i]
            L = cur[o] if st["kind"] == "listed" else np.arange(V)
            assert np.array_equal(L, e["L"])
            if f != "bank":
                inputs, controls = ss.launch_signals(f, V, st["n"], st["sig"], st.get("drain", False))
            for k, v in enumerate(L):
                w = singles[(o, int(v))]
                if f == "bank":
                    y, _, pk = w.run([0], st["n"])
                    ys = [y]
                else:
                    ys, _, pk = w.run([0], st["n"], {a: b[v:v + 1] for a, b in inputs.items()}, {a: b[v:v + 1] for a, b in controls.items()})
                for out, (mine, whole) in enumerate(zip(ys, e["ys"])):
                    assert_bits_equal(mine[0], whole[k], True, f"step {i} output {out} voice {v}")
                assert pk[0] == e["peaks"][k], (i, v)
        elif st["kind"] in ("updates", "steal"):
            for target, node, index, first, n, bits in st["records"]:
                for v in range(first, first + n):
                    singles[(o, v)].apply([(target, node, index, 0, 1, bits)])
            if st["kind"] == "steal" and st["L"] is not None:
                cur[o] = st["L"]
        elif st["kind"] == "move":
            if st["op"] == "export":
                slots[st["slot"]] = [singles[(o, int(v))].take([0])[0] for v in st["voices"]]
            else:
                for v, s in zip(st["voices"], slots[st["slot"]]):
                    singles[(o, int(v))].put([0], [s])
    worlds, _ = ss.walk_model(session)
    for o, w in worlds.items():
        t = w.tables()
        for v in range(w.V):
            one = singles[(o, v)]
            t1 = one.tables()
            for key, row in t.items():
                assert row[v] == t1[key][0], (o, v, key)
            if f != "bank":
                for key, a in w.st.items():
                    if w._voice_axis(key) == 0:      # rings and feedback vectors
                        assert_bits_equal(a[v], one.st[key][0], True, f"{o} voice {v} {key}")


# ---- update semantics -----------------------------------------------------------------------------------------------------------------------
def test_cleared_words_come_from_the_oracle():
    o = ss.oracle()
    assert cleared_words(o, Proc.INTEGER_DELAY) == {}
    assert cleared_words(o, Proc.FRACTIONAL_DELAY) == {1: 0, 2: 0}                  # the allpass section's x1, y1
    assert cleared_words(o, Proc.PITCHBENDABLE_DELAY) == {1: 0, 2: 0, 6: 0, 7: 0}
    assert cleared_words(o, Proc.LOPASS) == {0: 0, 1: 0} and cleared_words(o, Proc.GAIN) == {}


@pytest.mark.parametrize("family", ["string", "three_ring", "pitchbend"])
def test_clear_rings_of_everything_is_a_fresh_world(family):
    """A whole-range CLEAR_RINGS(-1) on a dirtied world: a fresh world with the params and coeffs kept, apart from the write indices
    (and the delay-time words a setter wrote, which clear() leaves alone like them)."""
    session = ss.make_session(0, family)
    V = session.shapes["B"]
    w, fresh = ss.new_world(family, V, session.tables["B"]), ss.new_world(family, V, session.tables["B"])
    inputs, controls = ss.launch_signals(family, V, 3, 1)
    ys, _, _ = w.run(np.arange(V), 3, inputs, controls)
    assert all(np.abs(y).max() > 0 for y in ys) and any(np.abs(a).max() > 0 for k, a in w.st.items() if k.endswith("/mem"))
    w.apply([(CLEAR_RINGS, -1, 0, 0, V, 0)])
    kept = 0
    for n in w.desc:
        if n["type"] == "proc" and n["kind"] in Proc.DELAYS:
            stay = [i for i in range(w.num_state(n["name"])) if i not in cleared_words(w.oracle, n["kind"])]
            assert all(i in stay for i in {Proc.PITCHBENDABLE_DELAY: (0, 5)}.get(n["kind"], (0,)))
            assert (w.st[n["name"]][0] == (3 * 64) % ss.RING).all(), "the write index stays"
            for i in stay:
                fresh.st[n["name"]][i] = w.st[n["name"]][i]
                kept += 1
    assert kept
    for key, a in w.st.items():
        assert_bits_equal(a, fresh.st[key], True, key)
    for key, a in w.params.items():
        assert_bits_equal(a, session.tables["B"]["params"][key], True, key)
    for key, a in w.coeffs.items():
        assert_bits_equal(a, session.tables["B"]["coeffs"][key], True, key)


def test_the_later_record_wins():
    session = ss.make_session(0, "string")
    w = ss.new_world("string", 80, session.tables["B"])
    w.apply([(PARAM, "g", 0, 10, 30, ss._f32(0.2)), (STATE, "fb", 5, 0, 80, 0x3C000000), (PARAM, "g", 0, 20, 5, ss._f32(0.3)), (CLEAR_RINGS, -1, 0, 30, 10, 0),
             (COEFF, "damp", 1, 0, 80, ss._f32(0.5)), (COEFF, "damp", 1, 79, 1, ss._f32(0.25))])
    g = w.params["g"]
    assert (g[10:20] == np.float32(0.2)).all() and (g[20:25] == np.float32(0.3)).all() and (g[25:40] == np.float32(0.2)).all()
    assert g[9] == session.tables["B"]["params"]["g"][9]
    fb = w.st["fb"].view(np.uint32)[:, 5]
    assert (fb[:30] == 0x3C000000).all() and (fb[30:40] == 0).all() and (fb[40:] == 0x3C000000).all()
    assert w.coeffs["damp"][1, 79] == np.float32(0.25) and (w.coeffs["damp"][1, :79] == np.float32(0.5)).all()
    bank = ss.new_world("bank", 80, ss.make_session(0, "bank").tables["B"])
    bank.state[:] = 9
    bank.apply([("input_const", 0, 0, 0, 80, ss._f32(0.01)), ("input_const", 0, 0, 40, 2, ss._f32(0.02)), (STATE, 1, 1, 0, 80, 7), ("clear", 1, 0, 3, 2, 0)])
    assert bank.in_const[40] == np.float32(0.02) and bank.in_const[42] == np.float32(0.01)
    assert (bank.state[bank.s0[1] + 1, 3:5] == 0).all() and bank.state[bank.s0[1] + 1, 5] == 7


# ---- what the default seeds reach --------------------------------------------------------------------------------------------------------
def survey(family):
    """Walk the family's default sessions through the model and note what happened."""
    seen = dict(kinds={k: 0 for k in ss.KINDS}, empty=False, all=False, moved_then_listed=False, steal_on_live_ring=False, relisted=False, silent=[])
    delay = ss.description(family)[3] if family != "bank" else 0
    for session in family_sessions(family):
        V = session.shapes
        cur = {o: np.zeros(0, np.uint32) for o in V}
        fresh_import = {o: set() for o in V}
        off = {o: np.full(n, -1, np.int64) for o, n in V.items()}          # launches spent off the list since last listed (-1: never listed)
        since_clear = {o: np.zeros(n, np.int64) for o, n in V.items()}   # DSPVectors run since a clear record (a new world is a cleared one)
        step_of = {}

        def on_launch(e, worlds):
            st = session.steps[e["step"]]
            o, L = e["obj"], e["L"].astype(np.int64)
            if st["kind"] == "listed":
                if fresh_import[o] & set(L.tolist()):
                    seen["moved_then_listed"] = True
                if (off[o][L] >= 2).any():
                    seen["relisted"] = True
                off[o][off[o] >= 0] += 1
                off[o][L] = 0
            fresh_import[o] -= set(L.tolist())
            for out, y in enumerate(e["ys"]):
                dead = np.flatnonzero(~(y != 0).any(1))
                still = worlds[o].in_const < np.float32(2.0 ** -64) if family == "bank" else np.zeros(V[o], bool)
                seen["silent"] += [(session.seed, e["step"], o, int(L[k]), out) for k in dead if since_clear[o][L[k]] >= delay and not still[L[k]]]
            since_clear[o][L] += e["n"]

        def on_step(i, st, worlds):
            o, kind = st["obj"], st["kind"]
            if kind != "move" or st["op"] == "import":
                seen["kinds"][kind] += 1
            if kind == "list" or (kind == "steal" and st["L"] is not None):
                seen["empty"] |= st["L"].size == 0
                seen["all"] |= st["L"].size == V[o]
            if kind == "steal" and family not in ("bank", "synth"):
                mem = [a for k, a in worlds[o].st.items() if k.endswith("/mem")]
                seen["steal_on_live_ring"] |= all(np.abs(a[st["voice"]]).max() > 0 for a in mem)
            if kind in ("updates", "steal"):
                for target, _, _, first, n, _ in st["records"]:
                    if target in ("clear", "clear_rings"):
                        since_clear[o][first:first + n] = 0
            if kind == "move":
                if st["op"] == "export":
                    step_of[st["slot"]] = since_clear[o][st["voices"].astype(np.int64)].copy()
                else:
                    fresh_import[o] |= set(int(v) for v in st["voices"])
                    since_clear[o][st["voices"].astype(np.int64)] = step_of[st["slot"]]
        ss.walk_model(session, on_launch, on_step=on_step)
    return seen


_surveys = {}


def surveyed(family):
    if family not in _surveys:
        _surveys[family] = survey(family)
    return _surveys[family]


@pytest.mark.parametrize("family", ss.FAMILIES)
def test_default_seeds_cover_what_the_fuzz_is_for(family):
    seen = surveyed(family)
    assert all(n >= 3 for n in seen["kinds"].values()), seen["kinds"]
    assert seen["empty"] and seen["all"] and seen["moved_then_listed"] and seen["relisted"], {k: v for k, v in seen.items() if k != "silent"}
    if family not in ("bank", "synth"):
        assert seen["steal_on_live_ring"]


@pytest.mark.parametrize("family", ss.FAMILIES)
def test_expected_rows_are_alive(family):
    """Every expected output row of a listed voice has a non-zero sample, but for voices cleared less than the case's largest total delay
    (in DSPVectors) before the launch - and for a bank voice whose frequency is below 2^-64 (the two slow-head lanes of the saw_odd
    chain): it stands still, a constant through a Bandpass, and dies away within a few DSPVectors whatever the session does."""
    silent = surveyed(family)["silent"]
    assert not silent, (len(silent), silent[:8])
