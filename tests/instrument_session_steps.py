"""Seeded random sessions of a polyphonic instrument bank as plain data (TEST INFRASTRUCTURE, no GPU): N instruments of P voices, one
voice graph with event rows over all V = N P voices, and the intended block of include/mlgpu.h walked for 12 blocks of 512 frames -
events, route_ahead, the sounding set, the tails' list, the listed launch, the note, clear_events - with every fourth block by
process_events on all voices, update records between the blocks and refused calls while a routed launch is pending.
tests/test_instrument_session_cpu.py walks them through the host model (instrument_session_model) alone,
tests/test_gpu_instrument_session.py through the device and the model side by side.

A session is a types.SimpleNamespace: family, seed, N, P, V, group (the group size of output 0, 0: none), mix (output 0 mixed down),
rows (the event rows the graph reads), cfg (the events object's settings as test_gpu_events.ref_run takes them), instruments (one event
list per instrument, times counted from the session's start), params / coeffs (the graph's tables after clear), all_listed (every
launch lists every voice: the sessions with drift), sounding_call, and blocks: dicts of
  index, plain (process_events on all voices instead of the listed call), launches [(n_vectors, start_offset)],
  updates (records as session_model takes them, applied before the block's events),
  refused {launch: (call, status name)}: a call that must be refused after that launch's route_ahead and change nothing."""
import types

import numpy as np

from madronalib_amd.constants import Op, Proc
from session_model import CLEAR, COEFF, PARAM
from test_gpu_events import BEND, CHAN_PRESS, CTRL, NOTE_OFF, NOTE_ON, performance

FAMILIES = ("midi4", "midi16", "mpe4", "mpe5", "drift")
SHAPES = {                                                    # the smallest shapes at which lanes, groups and wavefronts can go wrong
    "midi4": dict(N=40, P=4, group=4, mix=False),             # 160 voices: two and a half wavefronts, instruments across a wavefront border
    "midi16": dict(N=9, P=16, group=16, mix=False),           # 144 voices, groups of 16: the LDS sum
    "mpe4": dict(N=40, P=4, group=4, mix=False),              # G = 8 lanes per instrument in the events object, 320 lanes
    "mpe5": dict(N=26, P=5, group=0, mix=True),               # V = 130: the plain listed form and a mixed-down output
    "drift": dict(N=40, P=4, group=4, mix=False),             # as midi4, MIDI and MPE alternating by seed, drift 0.5
}
BLOCK, VECTORS, N_BLOCKS = 512, 8, 12
FRAMES = BLOCK * (N_BLOCKS + 1)          # the performances go on through one block more: the hand-over to mlgpu_events_process at the end
GLIDE, QUIET, HOLD = 0.01, 1e-4, 4
ROW_NAMES = ("pitch", "gate", "vox", "z", "x", "y", "mod")
SMALL = 2.0 ** -20                        # what the controller rows add to a voice's output: far below QUIET
REFUSED = (("route_ahead", "ERR_INVALID"), ("add_event", "ERR_INVALID"), ("other_n_vectors", "ERR_INVALID"), ("process_listed", "ERR_INVALID"))
_oracle = []


def oracle():
    if not _oracle:
        from cpu_checkers import Oracle
        _oracle.append(Oracle())
    return _oracle[0]


def _f32(x):
    return int(np.float32(x).view(np.uint32))


def is_mpe(family, seed):
    return family.startswith("mpe") or (family == "drift" and seed % 2 == 1)


def description(mpe):
    """(description, outputs) of the device graph: pitch -> exp2Approx x baseFreq -> SineGen, gate -> ADSR, z -> OnePole,
    out = osc env (0.5 + zs) + (the controller rows' sum) SMALL. Three nodes carry state that follows the list: osc, env, zs. Output 0 is
    `out` (group-summed or mixed down), output 1 the per-voice signal before the controller rows are added."""
    rows = range(7) if mpe else (0, 1, 3, 6)
    d = [dict(name=ROW_NAMES[r], type="event_row", kind=r) for r in rows]
    op = lambda name, kind, *ins: dict(name=name, type="op", kind=kind, inputs=list(ins))     # noqa: E731
    d += [dict(name="baseFreq", type="param"), dict(name="half", type="const", value=0.5), dict(name="small", type="const", value=SMALL),
          op("ratio", Op.EXP2_APPROX, "pitch"), op("freq", Op.MULTIPLY, "ratio", "baseFreq"),
          dict(name="osc", type="proc", kind=Proc.SINE_GEN, inputs=["freq"]), dict(name="env", type="proc", kind=Proc.ADSR, inputs=["gate"]),
          dict(name="zs", type="proc", kind=Proc.ONE_POLE, inputs=["z"]),
          op("level", Op.ADD, "half", "zs"), op("tone", Op.MULTIPLY, "osc", "env"), op("voice", Op.MULTIPLY, "tone", "level")]
    ctl = "mod"
    if mpe:       # ((mod + x) + y) + vox
        d += [op("c0", Op.ADD, "mod", "x"), op("c1", Op.ADD, "c0", "y"), op("c2", Op.ADD, "c1", "vox")]
        ctl = "c2"
    d += [op("side", Op.MULTIPLY, ctl, "small"), op("out", Op.ADD, "voice", "side")]
    return d, ["out", "voice"]


def onepole_sets(n=8):
    return np.stack([oracle().make_coeffs("onepole", 0.02 + 0.2 * j / n) for j in range(n)], 1).astype(np.float32)


# ---- the performances ------------------------------------------------------------------------------------------------------------------------
def _held_at_end(evs):
    held = []
    for e in evs:
        if e[0] == NOTE_ON:
            held.append((e[1], e[2]))
        elif e[0] == NOTE_OFF and (e[1], e[2]) in held:
            held.remove((e[1], e[2]))
        elif e[0] == CTRL and e[2] == 123:
            held = []
    return held


def _channel_one(rng, t):
    r = rng.random()
    if r < 0.4:
        return (CTRL, 1, int(rng.choice([16, 73, 74])), t, float(np.float32(rng.random())), 0.0)
    if r < 0.7:
        return (BEND, 1, 0, t, float(np.float32(rng.uniform(-1, 1))), 0.0)
    return (CHAN_PRESS, 1, 0, t, float(np.float32(rng.random())), 0.0)


def _window(rng, kind, P, a, b, density, seed, burst):
    """The mod controller, then test_gpu_events.performance between the frames a and b (`density` of them laid over each other), every
    note still held at b released there; under MPE channel-1 controllers, bends and pressure through the window and three more in the release tails after it."""
    evs = [(CTRL, 1, 16, a, float(np.float32(rng.uniform(0.25, 0.75))), 0.0)]
    if burst:       # P short notes at once (under MPE on P channels): every voice of the instrument sounds once
        for j in range(P):
            t, c = a + 3 * j, (2 + j if kind == "mpe" else 1)
            evs += [(NOTE_ON, c, 36 + j, t, float(np.float32((j - 12) / 12.0)), float(np.float32(0.3 + 0.04 * j))), (NOTE_OFF, c, 36 + j, t + int(rng.integers(40, 200)), 0.0, 0.0)]
    for j in range(density):
        evs += [(e[0], e[1], e[2], e[3] + a, e[4], e[5]) for e in performance(kind, seed * 7 + j, b - a, P)]
    evs.sort(key=lambda e: e[3])
    evs += [(NOTE_OFF, c, k, b, 0.0, 0.0) for c, k in _held_at_end(evs)]
    if kind == "mpe":
        t = a + int(rng.integers(0, 200))
        while t < b:
            evs.append(_channel_one(rng, t))
            t += int(rng.integers(20, 300))
        evs += [_channel_one(rng, min(FRAMES - 1, b + dt)) for dt in (int(rng.integers(20, 80)), int(rng.integers(150, 300)), int(rng.integers(400, 520)))]
    return evs


def instrument_events(family, seed, i, mpe):
    """Instrument i's events. Two waves with silence between them, so that the lists fill, empty and fill again: the first wave's windows
    lie in blocks 0 .. 3, the second wave's begin in blocks 9 and 10 and last to the end."""
    s = SHAPES[family]
    rng = np.random.default_rng([seed, FAMILIES.index(family), i, 17])
    kind, density = ("mpe" if mpe else "midi"), (4 if s["P"] == 16 else 1)
    first = rng.random() < 0.85
    evs = []
    if first:
        a = int(rng.integers(0, 3 * BLOCK // 2))
        b = min(a + int(rng.integers(3 * BLOCK // 2, 3 * BLOCK)), 4 * BLOCK)
        evs += _window(rng, kind, s["P"], a, b, density, 1000 * seed + 10 * i, True)
    if not first or rng.random() < 0.3:
        a = int(rng.integers(9 * BLOCK, 21 * BLOCK // 2))
        evs += _window(rng, kind, s["P"], a, FRAMES - BLOCK // 4, density, 1000 * seed + 10 * i + 5, not first)
    return sorted(evs, key=lambda e: e[3])       # (stable: events of one frame keep their order)


# ---- the generator ---------------------------------------------------------------------------------------------------------------------------
def _cuts(rng):
    """A block of VECTORS DSPVectors in 1 to 3 launches of random vector counts: [(n_vectors, start_offset)]."""
    k = int(rng.integers(1, 4))
    at = sorted(rng.choice(np.arange(1, VECTORS), k - 1, replace=False).tolist()) if k > 1 else []
    edges = [0] + at + [VECTORS]
    return [(edges[j + 1] - edges[j], 64 * edges[j]) for j in range(k)]


def _run_across_64(V, rng):
    b = 64 * int(rng.integers(1, (V - 1) // 64 + 1))
    first = b - int(rng.integers(1, 12))
    return first, min(V, b + int(rng.integers(1, 12))) - first


def _updates(V, rng, sets):
    recs = []
    if rng.random() < 0.6:        # a steal: the voice cleared and retuned
        v = int(rng.integers(0, V))
        recs += [(CLEAR, -1, 0, v, 1, 0), (PARAM, "baseFreq", 0, v, 1, _f32(rng.uniform(0.004, 0.03)))]
    if rng.random() < 0.6:        # a run of voices across a 64-voice border retuned
        first, n = _run_across_64(V, rng)
        recs.append((PARAM, "baseFreq", 0, first, n, _f32(rng.uniform(0.004, 0.03))))
    if rng.random() < 0.4:        # ... and another smoothing of z for such a run
        first, n = _run_across_64(V, rng)
        recs.append((COEFF, "zs", 0, first, n, _f32(sets[0, int(rng.integers(0, sets.shape[1]))])))
    return recs


def make_session(seed, family, updates=True):
    s = SHAPES[family]
    N, P = s["N"], s["P"]
    V = N * P
    mpe = is_mpe(family, seed)
    drift = 0.5 if family == "drift" else 0.0
    rng = np.random.default_rng([seed, FAMILIES.index(family), 99])
    sets = onepole_sets()
    adsr = oracle().make_coeffs("adsr", 0.001, 0.01, 0.7, 0.03, 48000.0).astype(np.float32)     # a release of some 550 samples that ends in exact zeros
    params = {"baseFreq": (440.0 / 48000.0 * 2.0 ** rng.uniform(-1.0, 1.0, V)).astype(np.float32)}
    coeffs = {"env": np.repeat(adsr[:, None], V, 1).copy(), "zs": sets[:, rng.integers(0, sets.shape[1], V)].copy()}
    blocks = []
    for b in range(N_BLOCKS):
        launches = _cuts(rng)
        refused = {k: REFUSED[int(rng.integers(0, len(REFUSED)))] for k in range(len(launches)) if rng.random() < 0.25}
        blocks.append(dict(index=b, plain=b % 4 == 3, launches=launches, updates=_updates(V, rng, sets) if updates and b else [], refused=refused))
    desc, outputs = description(mpe)
    return types.SimpleNamespace(
        family=family, seed=seed, N=N, P=P, V=V, mpe=mpe, group=s["group"], mix=s["mix"], rows=tuple(n["kind"] for n in desc if n["type"] == "event_row"),
        cfg=dict(polyphony=P, mpe=int(mpe), glide=GLIDE, drift=drift, bend=7.0, mpe_bend=48.0, mod_cc=16),
        instruments=[instrument_events(family, seed, i, mpe) for i in range(N)], params=params, coeffs=coeffs, blocks=blocks,
        all_listed=drift > 0.0, sounding_call="sounding_voices" if (not mpe and seed % 2 == 1) else "sounding_graph_voices",
        desc=desc, outputs=outputs)


def default_cases(first=0, count=None, families=FAMILIES):
    """[(family, seed)]: two seeds per family."""
    return [(f, first + i) for f in families for i in range(count or 2)]
