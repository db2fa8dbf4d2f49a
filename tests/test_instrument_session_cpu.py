"""The host model of an instrument-bank session (instrument_session_model) pinned, and every default session of
instrument_session_steps held to liveness conditions computed from the model alone. No GPU. The event rows come from the reference's own
EventsToSignals class in oracle/_ref/libdropin_ref.so, which the build makes; without it the whole file skips, loudly."""
import os
import warnings

import numpy as np
import pytest

import graph_oracle
import instrument_session_model as ism
import instrument_session_steps as iss
from inputs import assert_bits_equal
from madronalib_amd.constants import Proc
from test_gpu_events import ROOT
from voice_list_groups_cases import expected_listed_groups

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libdropin_ref.so")
if not os.path.exists(REF_SO):
    warnings.warn("oracle/_ref/libdropin_ref.so is not here: the instrument-session model was NOT pinned and no session was checked")
    pytest.skip("oracle/_ref/libdropin_ref.so not available here", allow_module_level=True)

CASES = iss.default_cases()
_walks = {}


def walked(family, seed):
    if (family, seed) not in _walks:
        session = iss.make_session(seed, family)
        _walks[family, seed] = (session,) + ism.walk(session)
    return _walks[family, seed]


def test_default_cases():
    assert len(CASES) == 2 * len(iss.FAMILIES) and {f for f, _ in CASES} == set(iss.FAMILIES)
    for f, seed in CASES:
        s = iss.make_session(seed, f)
        assert s.V == s.N * s.P and len(s.blocks) == iss.N_BLOCKS and all(sum(n for n, _ in b["launches"]) == iss.VECTORS for b in s.blocks)
        assert all(off == 64 * sum(n for n, _ in b["launches"][:k]) for b in s.blocks for k, (_, off) in enumerate(b["launches"]))
        assert [b["plain"] for b in s.blocks] == [i % 4 == 3 for i in range(iss.N_BLOCKS)]
        assert all(0 <= e[3] < iss.FRAMES for evs in s.instruments for e in evs)
        assert s.all_listed == (f == "drift") and (s.cfg["drift"] > 0) == (f == "drift")
    assert iss.make_session(0, "drift").mpe != iss.make_session(1, "drift").mpe


# ---- the model pinned ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", iss.FAMILIES)
def test_with_all_voices_listed_the_model_is_one_evaluate_of_the_whole_graph(family):
    """No update records, every launch with every voice: the launches' outputs laid end to end are ONE graph_oracle.evaluate of the
    whole graph over the session's 96 DSPVectors on the reference's rows; the group rows and the mixed-down row are the checker's of
    those; the state afterwards is that evaluate's."""
    session = iss.make_session(0, family, updates=False)
    session.all_listed = True
    world, launches = ism.walk(session)
    o, V, T = iss.oracle(), session.V, iss.N_BLOCKS * iss.VECTORS
    rows = ism.reference_rows(session)
    desc = ism.model_description(session.desc)
    states = {n["name"]: o.chain_clear([n["kind"]], V) for n in desc if n["type"] == "proc"}
    whole = graph_oracle.evaluate(o, desc, session.outputs, V, T, {iss.ROW_NAMES[r]: rows[r][:, :64 * T] for r in session.rows}, session.params, session.coeffs, states)
    everyone = np.arange(V)
    assert sum(e["n"] for e in launches) == T
    for e in launches:
        at = slice(e["f0"], e["f0"] + 64 * e["n"])
        what = f"{family} block {e['block']} launch {e['k']}"
        assert np.array_equal(e["L"], everyone)
        for i, y in enumerate(e["ys"]):
            assert_bits_equal(y, whole[i][:, at], True, f"{what}: output {i}")
        if session.group:
            assert_bits_equal(e["groups"][0], expected_listed_groups(o, np.ascontiguousarray(whole[0][:, at]), everyone, session.group)[0], True, f"{what}: group rows")
        if session.mix:
            assert_bits_equal(e["mix"][0], o.mixdown(np.ascontiguousarray(whole[0][:, at]), None), True, f"{what}: mixed-down row")
    for name, st in states.items():
        assert_bits_equal(world.st[name], st, False, f"{family}: state of {name}")
    assert np.abs(whole[0]).max() > 0.01


@pytest.mark.parametrize("family", iss.FAMILIES)
def test_a_voice_of_the_model_is_a_one_voice_model(family):
    """A sample of voices, each walked alone through seed 1's session - its update records, the launches that list it, its rows - as a
    world of one voice: the V-voice model's rows and peaks at its list positions, and its state at the end."""
    session, world, launches = walked(family, 1)
    V, rows = session.V, ism.reference_rows(session)
    touched = {v for b in session.blocks for r in b["updates"] for v in (r[3], r[3] + r[4] - 1)}
    sample = sorted({0, 3, 63, 64, V - 1} | set(np.random.default_rng(5).choice(V, 6, replace=False).tolist()) | set(sorted(touched)[:6]))
    by_block = {}
    for e in launches:
        by_block.setdefault(e["block"], []).append(e)
    ran = skipped = 0
    for v in sample:
        one = ism.new_world(session, voices=[v])
        for blk in session.blocks:
            one.apply([(t, node, i, 0, 1, bits) for t, node, i, first, n, bits in blk["updates"] if first <= v < first + n])
            for e in by_block[blk["index"]]:
                at = np.flatnonzero(e["L"] == v)
                if not at.size:
                    skipped += 1
                    continue
                ran += 1
                ys, _, peaks = one.run([0], e["n"], {iss.ROW_NAMES[r]: rows[r][v:v + 1, e["f0"]:e["f0"] + 64 * e["n"]] for r in session.rows})
                for i, y in enumerate(ys):
                    assert_bits_equal(y[0], e["ys"][i][at[0]], True, f"{family} voice {v} block {e['block']} launch {e['k']}: output {i}")
                assert peaks[0] == e["peaks"][at[0]]
        got, want = one.tables(), world.tables()
        for key in want:
            assert got[key][0] == want[key][v], f"{family} voice {v}: {key}"
    assert ran > 0 and (skipped > 0 or session.all_listed)


def test_a_clear_record_leaves_the_envelope_but_its_segment():
    session = iss.make_session(0, "midi4")
    w = ism.new_world(session)
    w.st["env"][:] = np.arange(8, dtype=np.uint32)[:, None] + 100
    w.st["zs"][:] = 7
    w.apply([("clear", -1, 0, 5, 2, 0)])
    assert (w.st["env"][:7] == np.arange(7, dtype=np.uint32)[:, None] + 100).all() and (w.st["env"][7, 5:7] == 4).all() and (w.st["env"][7, :5] == 107).all()
    assert (w.st["zs"][:, 5:7] == 0).all() and (w.st["zs"][:, :5] == 7).all()
    assert iss.oracle().chain_clear([Proc.ADSR], 1)[:7].max() == 0


# ---- liveness: computed from the model alone ------------------------------------------------------------------------------------------------
def loud(e):
    return e["peaks"].astype(np.uint64) > ism.QUIET_BITS


@pytest.mark.parametrize("family,seed", CASES, ids=lambda c: str(c))
def test_liveness(family, seed):
    """What a session must do for its comparison to mean something. A session of the drift family lists every voice in every launch, so
    the conditions on changing lists are those of the other families."""
    session, world, launches = walked(family, seed)
    rows, G, V = ism.reference_rows(session), session.group, session.V
    listed = [e for e in launches if not e["plain"]]
    sets = [set(e["L"].tolist()) for e in listed]
    if not session.all_listed:
        # voices enter, stay listed while their model peak exceeds the threshold, and leave
        assert any(b - a for a, b in zip(sets, sets[1:])) and any(a - b for a, b in zip(sets, sets[1:]))
        for e, nxt in zip(listed, sets[1:]):
            assert set(e["L"][loud(e)].tolist()) <= nxt, f"block {e['block']} launch {e['k']}: a loud voice left"
        sizes = [len(s) for s in sets]
        assert min(sizes) == 0 and max(sizes) > 64, sizes
        assert any(n == 0 and max(sizes[:i], default=0) > 0 and max(sizes[i:]) > 0 for i, n in enumerate(sizes)), sizes      # an empty list between two waves
        if family == "mpe5":
            assert any(len(e["L"]) > 64 and e["L"][63] // 5 == e["L"][64] // 5 for e in listed), "no list's positions 63 and 64 are one instrument's voices"
    else:
        assert all(len(s) == V for s in sets)
    # a note-on lands on a voice whose release is still listed: gate zero at the end of the launch before, loud there, gate up in this one
    retriggered = 0
    for p, e in zip(launches, launches[1:]):
        if p["plain"] or e["plain"]:
            continue
        quiet_gate = rows[1][:, e["f0"] - 1] == 0
        up = np.any(rows[1][:, e["f0"]:e["f0"] + 64 * e["n"]] != 0, axis=1)
        tails = p["L"][loud(p)]
        retriggered += int(np.sum(quiet_gate[tails] & up[tails] & np.isin(tails, e["L"])))
    assert retriggered > 0, "no note-on lands on a voice whose release is still listed"
    # a listed wavefront mixes voices of four or more instruments
    assert any(len({v // session.P for v in w}) >= 4 for e in listed for w in ism.listed_wavefronts(e["L"], G))
    # under MPE a channel-1 event arrives while only release tails of that instrument are listed
    if session.mpe:
        found = 0
        for e in listed:
            gate_up = np.any(rows[1][:, e["f0"]:e["f0"] + 64 * e["n"]] != 0, axis=1)
            for i in ism.instruments_with_events(session, e["f0"], e["n"]):
                if not any(ev[1] == 1 and e["f0"] <= ev[3] < e["f0"] + 64 * e["n"] for ev in session.instruments[i]):
                    continue
                mine = (e["L"] // session.P) == i
                found += int(mine.any() and not gate_up[e["L"][mine]].any() and loud(e)[mine].any())
        assert found > 0, "no channel-1 event arrives while only release tails of its instrument are listed"
    # every group-summed row, the mixed-down row and every voice's peak are non-zero somewhere
    peak = np.zeros(V, np.uint32)
    for e in launches:
        peak[e["L"]] = np.maximum(peak[e["L"]], e["peaks"])
    assert peak.min() > 0, f"voices {np.flatnonzero(peak == 0)[:8]} never give a non-zero sample"
    if G:
        top = np.zeros(V // G, np.float32)
        for e in launches:
            if e["M"].size:
                top[e["M"]] = np.maximum(top[e["M"]], np.abs(e["groups"][0]).max(axis=1))
        assert top.min() > 0, f"instruments {np.flatnonzero(top == 0)[:8]} never give a non-zero sum"
    if session.mix:
        assert max(np.abs(e["mix"][0]).max() for e in launches) > 0
    # some voice is stolen, and some call is refused
    assert any(b["refused"] for b in session.blocks) and any(r[0] == "clear" for b in session.blocks for r in b["updates"])
