"""Graphs, lists and expected values of a graph's listed group sums (mlgpu_graph_enable_voice_list_groups, _reserve_voice_list_groups,
_process_listed_groups), shared by tests/test_graph_voice_list_groups_cpu.py and tests/test_gpu_graph_voice_list_groups.py.

The rule: a group-summed output of the call has one row per LISTED instrument - the distinct L[i] // G, ascending - which is
((0 + y[a0]) + y[a1]) + ... over that instrument's listed voices in voice order, y the float mlgpu_graph_process_listed would store.
So the expected rows are graph_voice_list_cases.expected_listed's rows of that output, accumulated per segment from +0.0 with the
CPU checker's float32 add (voice_list_groups_cases.expected_listed_groups); every plain output and the peaks are expected_listed's
and expected_peaks' by list position. For a graph with rings y comes from a plain K-voice graph on the device instead."""
import types

import numpy as np

from graph_voice_list_cases import T, V, expected_listed, expected_peaks, gain_desc, gathered, load_tables, ring_case, synth_case   # noqa: F401
from voice_list_groups_cases import GROUPS, PLAN_TABLE, expected_listed_groups, group_lists, model_plan   # noqa: F401

LISTS = group_lists()
assert V == 2352 and T == 3 and V % 16 == 0


def build_group_graph(engine, case, sums, n_voices=V, switch=True, voice_lists=False, delay_windows=False, compile_now=True):
    """The case's graph over n_voices voices with the outputs of `sums` {output index: G} summed by groups of G voices and, with
    `switch`, the listed form by the lane plan (voice_lists: the plain listed form instead). No mixdowns: case.mix is not applied."""
    import madronalib_amd as ml
    g = ml.Graph(engine, n_voices, case.desc, case.outputs, delay_windows=delay_windows, compile_now=False, voice_lists=voice_lists,
                 voice_list_groups=switch, output_groups=dict(sums), input_groups={list(case.inputs).index(k): p for k, p in case.groups.items()})
    if compile_now and engine.h is not None:
        g.compile()
    return g


def offline_case(desc_outputs, groups=None):
    """A case with nothing per voice: what build_group_graph needs to make an engine-less graph."""
    desc, outputs = desc_outputs
    return types.SimpleNamespace(desc=desc, outputs=outputs, mix=(), inputs={n["name"]: None for n in desc if n["type"] == "input"}, groups=groups or {})


def expected_plan(lname, G):
    """(N lanes, pads, J, M) of the list's lane plan: model_plan, which must agree with PLAN_TABLE where the table has the pair."""
    L = LISTS[lname]
    _, N, pads, J = model_plan(L, G)
    if (lname, G) in PLAN_TABLE:
        assert PLAN_TABLE[(lname, G)] == (N, pads, J)
    M = np.unique(L.astype(np.int64) // G).astype(np.uint32)
    assert M.size == J
    return N, pads, J, M


def expected_outputs(oracle, ys, L, sums, flush=False):
    """expected_listed's signals -> what the call stores: [J][S] for an output of `sums`, [K][S] for every other one."""
    return [expected_listed_groups(oracle, y, L, sums[o], flush=flush)[0] if o in sums else y for o, y in enumerate(ys)]


def minus_zero_case(oracle):
    """A Gain (positive per-voice coefficients) on a streamed input whose rows of voices 5 and 40 are -0.0 throughout: their outputs are
    -0.0. In the list, at G = 4, voice 5 is the only listed voice of instrument 1 - its row must be +0.0 -, voice 40 shares instrument
    10 with voice 41, an ordinary one, and instrument 2 is listed in full."""
    desc, outputs = gain_desc()
    rng = np.random.default_rng(77)
    x = (rng.uniform(-1.0, 1.0, (V, 64 * T))).astype(np.float32)
    x[[5, 40]] = np.float32(-0.0)
    gain = rng.uniform(0.25, 1.0, (1, V)).astype(np.float32)
    case = types.SimpleNamespace(desc=desc, outputs=outputs, mix=(), inputs={"x": x}, groups={}, controls={}, params={}, coeffs={"gain": gain},
                                 states={"gain": oracle.chain_default_state([desc[1]["kind"]], V)})
    L = np.array([0, 1, 5, 8, 9, 10, 11, 40, 41, 2351], np.uint32)
    return case, L
