"""Seeded random sessions of a live voice bank as plain data (TEST INFRASTRUCTURE, no GPU): the object shapes, the initial tables and a
list of steps - voice lists, listed and plain launches, update records, steals, voice moves, refused calls. tests/test_session_model_cpu.py
walks them through the host model (session_model) alone, tests/test_gpu_session_fuzz.py through the device and the model side by side.

Two objects of one signature take part: A (the large shape) and its partner B. A step is a dict:
  list     obj, L                            a new voice list
  listed   obj, n, sig, mixdown, gains       process_listed (a bank: process_listed_mixdown with per-voice gains when `mixdown`)
  plain    obj, n, sig                       process of all voices
  updates  obj, records                      one apply_updates call (records as session_model takes them)
  steal    obj, voice, records, L            the documented block: clear the voice, retune it, list it
  move     op "export" | "import", obj, voices, slot      records into / out of record buffer `slot`
  refused  obj, call, status                 a call that must be refused with Status.<status> and change nothing
`sig` seeds the launch's input rows (launch_signals), `gains` the mixdown gains (launch_gains)."""
import types

import numpy as np

import graph_voice_list_cases as gcases
from inputs import lcg_noise
from madronalib_amd.constants import Proc
from session_model import CLEAR, CLEAR_RINGS, COEFF, INPUT_CONST, PARAM, STATE, BankWorld, GraphWorld

FAMILIES = ("bank", "synth", "string", "three_ring", "pitchbend")
KINDS = ("list", "listed", "plain", "updates", "steal", "move", "refused")
SHAPES = {"bank": (2352, 80)}       # every graph family: 600 (three 256-voice blocks, the last one partial) and 80 (a last wavefront of 16)
WARMUP = 4                          # DSPVectors of all voices before the first step: rings of 256 samples are full
RING, DRAIN_DELAY = 256, 192.0     # every ring is 256 samples long; the longest delay time a ring of 256 serves
BANK_PROCS = [Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN]
_oracle = []


def oracle():
    if not _oracle:
        from cpu_checkers import Oracle
        _oracle.append(Oracle())
    return _oracle[0]


def shapes(family):
    return SHAPES.get(family, (600, 80))


def pitchbend_desc():
    """One PitchbendableDelay on a streamed input, its delay time a streamed per-voice input too."""
    return [dict(name="x", type="input"), dict(name="dt", type="input"),
            dict(name="pb", type="proc", kind=Proc.PITCHBENDABLE_DELAY, inputs=["x", "dt"], max_delay=180.0)], ["pb"]


def description(family):
    """(description, outputs, mixed-down outputs, the case's largest total delay in DSPVectors)."""
    if family == "synth":
        return gcases.synth_desc() + ((1,), 0)
    if family == "string":
        return gcases.string_desc() + ((), 2)
    if family == "three_ring":
        return gcases.three_ring_desc() + ((), 6)
    if family == "pitchbend":
        return pitchbend_desc() + ((), 3)
    raise KeyError(family)


def _f32(x):
    return int(np.float32(x).view(np.uint32))


# ---- the initial tables ---------------------------------------------------------------------------------------------------------------------
def _coefficient_sets(name, n=16):
    o = oracle()
    if name == "lopass":
        return np.stack([o.make_coeffs("lopass", 0.02 + 0.28 * j / n, 0.7) for j in range(n)], 1).astype(np.float32)
    if name == "onepole":
        return np.stack([o.make_coeffs("onepole", 0.05 + 0.35 * j / n) for j in range(n)], 1).astype(np.float32)
    if name == "bandpass":
        return np.stack([o.make_coeffs("bandpass", 0.02 + 0.3 * j / n, 0.6) for j in range(n)], 1).astype(np.float32)
    raise KeyError(name)


def irregular(V):
    """(unequal, odd, dense) voices of a synth of V voices, graph_voice_list_cases.irregular_voices' kinds sprinkled over the shape: saw and
    pulse phase counters that differ, a pulse width outside [0, 1], a frequency too high for a trip."""
    v = np.arange(V)
    return v[v % 37 == 11], v[v % 53 == 20], v[v % 61 == 30]


def initial_tables(family, V, seed):
    rng = np.random.default_rng([seed, V, FAMILIES.index(family)])
    if family == "bank":
        sets = _coefficient_sets("bandpass")
        coeffs = np.concatenate([sets[:, (np.arange(V) * 7 + seed) % 16], np.full((1, V), 0.25, np.float32)], 0)
        in_const = (55.0 * 2.0 ** (5.0 * rng.random(V)) / 48000.0).astype(np.float32)
        if seed % 2:     # voice_list_cases' saw_odd: a frequency below 2^-64 in one lane of the first wavefront and one of the last
            in_const[[5, V - 3]] = np.float32(1e-30)
        # nothing from clear: per-voice phases and filter memories (a voice at such a frequency is silent from clear for good)
        state = np.concatenate([rng.integers(0, 2 ** 32, (1, V), dtype=np.uint64).astype(np.uint32), rng.uniform(-0.2, 0.2, (2, V)).astype(np.float32).view(np.uint32)], 0)
        return dict(coeffs=np.ascontiguousarray(coeffs, np.float32), in_const=in_const, state=np.ascontiguousarray(state))
    if family == "synth":
        unequal, odd, dense = irregular(V)
        freq = rng.uniform(0.001, 0.05, V).astype(np.float32)
        freq[dense] = np.float32(0.21)
        width = rng.uniform(0.1, 0.9, V).astype(np.float32)
        width[odd] = np.float32(1.5)
        phase = rng.integers(0, 2 ** 32, V, dtype=np.uint64).astype(np.uint32)
        other = phase.copy()
        other[unequal] += np.uint32(0x12345678)
        return dict(params={"freq": freq}, coeffs={"pulse": width[None, :].copy(), "lp": _coefficient_sets("lopass")[:, rng.integers(0, 16, V)]},
                    states={"saw": phase[None, :].copy(), "pulse": other[None, :].copy(), "lp": rng.uniform(-0.2, 0.2, (2, V)).astype(np.float32).view(np.uint32).copy()})
    if family == "pitchbend":
        return dict(params={}, coeffs={}, states={})
    params = {"dt": rng.uniform(1.0, 95.0, V).astype(np.float32), "g": rng.uniform(0.5, 0.95, V).astype(np.float32)}
    coeffs = {}
    if family == "string":
        coeffs["damp"] = _coefficient_sets("onepole")[:, rng.integers(0, 16, V)]
    else:
        params["dt2"] = rng.uniform(1.0, 170.0, V).astype(np.float32)
    return dict(params=params, coeffs=coeffs, states={})


def new_world(family, V, tables):
    if family == "bank":
        w = BankWorld(oracle(), BANK_PROCS, V)
        w.load(tables["coeffs"], tables["in_const"], tables["state"])
        return w
    desc, outputs, mix, _ = description(family)
    w = GraphWorld(oracle(), desc, outputs, V, mix)
    w.load(tables["params"], tables["coeffs"], tables["states"])
    return w


# ---- a launch's inputs ----------------------------------------------------------------------------------------------------------------------
def launch_signals(family, V, n, sig, drain=False):
    """(inputs {name: [V][64 n]}, controls {name: [V][n]}) of the launch seeded `sig`: V rows whatever the list. drain: a streamed delay
    time stands at DRAIN_DELAY."""
    if family == "bank":
        return {}, {}
    x = lcg_noise(np.arange(V, dtype=np.uint32) * np.uint32(7) + np.uint32(sig * 1009 + 3), 64 * n)
    if family == "synth":
        amp = np.random.default_rng([sig, V]).uniform(0.2, 1.0, (V, n)).astype(np.float32)
        return {"x": x * np.float32(0.25)}, {"amp": amp}
    if family == "pitchbend":   # a delay time that moves through the launch, another ramp in every voice: 1 .. 180 samples
        v, s = np.arange(V)[:, None], np.arange(64 * n)[None, :]
        dt = 90.0 + 85.0 * np.sin(0.37 * v + 0.11 * sig + 0.004 * (1 + v % 5) * s)
        return {"x": x, "dt": np.full((V, 64 * n), DRAIN_DELAY, np.float32) if drain else np.clip(dt, 1.0, 180.0).astype(np.float32)}, {}
    return {"x": x}, {}


def launch_gains(V, seed):
    g = np.random.default_rng([seed, V, 77]).uniform(-1, 1, V).astype(np.float32)
    g[1], g[V - 2] = np.float32(-0.0), np.float32(1e-40)
    return g


# ---- the generator --------------------------------------------------------------------------------------------------------------------------
def _run_across(V, rng, boundary):
    """(first, n) of a run of voices across a multiple of `boundary` inside V (V <= boundary: across 64)."""
    if V <= boundary:
        boundary = 64
    b = boundary * int(rng.integers(1, (V - 1) // boundary + 1))
    first = b - int(rng.integers(1, 20))
    return first, min(V, b + int(rng.integers(1, 20))) - first


LIST_KINDS = ("empty", "first", "last", "wave", "run64", "run256", "p5", "p50", "p95", "all")


def _draw_list(V, rng, kind=None):
    kind = kind or LIST_KINDS[int(rng.integers(0, len(LIST_KINDS)))]
    if kind == "empty":
        L = []
    elif kind == "first":
        L = [0]
    elif kind == "last":
        L = [V - 1]
    elif kind == "wave":      # exactly one wavefront of scattered voices
        L = np.arange(0, 64 * (V // 64), V // 64) if V >= 128 else rng.choice(V, 64, replace=False)
    elif kind in ("run64", "run256"):
        first, n = _run_across(V, rng, 64 if kind == "run64" else 256)
        L = np.arange(first, first + n)
    elif kind == "all":
        L = np.arange(V)
    else:
        L = np.flatnonzero(rng.random(V) < {"p5": 0.05, "p50": 0.5, "p95": 0.95}[kind])
    return kind, np.sort(np.asarray(L, np.int64)).astype(np.uint32)


class _Knobs:
    """What the update records of one family may write, and with which values."""

    def __init__(self, family):
        self.family = family
        f = family
        u = lambda lo, hi: (lambda rng: _f32(rng.uniform(lo, hi)))             # noqa: E731
        phase = lambda rng: int(rng.integers(0, 2 ** 32))                        # noqa: E731
        mem = u(-0.2, 0.2)
        self.ring_nodes, self.plain_nodes, self.sets = [], [], {}
        if f == "bank":
            self.words = [(INPUT_CONST, 0, 0, u(0.001, 0.05)), (COEFF, 2, 0, u(0.1, 0.5)), (STATE, 0, 0, phase), (STATE, 1, 0, mem), (STATE, 1, 1, mem)]
            self.sets = {1: _coefficient_sets("bandpass")}
            self.plain_nodes = [0, 1, -1]
        elif f == "synth":
            self.words = [(PARAM, "freq", 0, u(0.001, 0.05)), (PARAM, "freq", 0, u(0.2, 0.24)), (COEFF, "pulse", 0, u(0.1, 0.9)), (COEFF, "pulse", 0, u(1.2, 1.6)),
                          (STATE, "saw", 0, phase), (STATE, "pulse", 0, phase), (STATE, "lp", 0, mem), (STATE, "lp", 1, mem)]
            self.sets = {"lp": _coefficient_sets("lopass")}
            self.plain_nodes = ["saw", "pulse", "lp", -1]
        elif f == "string":
            self.words = [(PARAM, "dt", 0, u(1.0, 95.0)), (PARAM, "g", 0, u(0.5, 0.95)), (STATE, "damp", 0, mem), (STATE, "line", 1, mem), (STATE, "line", 2, mem)]
            self.words += [(STATE, "fb", i, mem) for i in (0, 17, 63)]
            self.sets = {"damp": _coefficient_sets("onepole")}
            self.ring_nodes, self.plain_nodes = ["line", -1], ["damp", "fb"]
        elif f == "three_ring":
            self.words = [(PARAM, "dt", 0, u(1.0, 95.0)), (PARAM, "dt2", 0, u(1.0, 170.0)), (PARAM, "g", 0, u(0.5, 0.95)), (STATE, "d2", 1, mem), (STATE, "d2", 2, mem)]
            self.words += [(STATE, "fb", i, mem) for i in (0, 31, 63)]
            self.ring_nodes, self.plain_nodes = ["d1", "d2", "d3", -1], ["fb"]
        elif f == "pitchbend":
            self.words = [(STATE, "pb", i, mem) for i in (1, 2, 6, 7)]
            self.ring_nodes = ["pb", -1]
        self.retune = [w for w in self.words if w[0] in (PARAM, COEFF, INPUT_CONST)]

    def voice_range(self, V, rng):
        r = rng.random()
        if r < 0.4:
            return int(rng.integers(0, V)), 1
        if r < 0.8:
            return _run_across(V, rng, 256)
        return 0, V

    def records(self, V, rng, count):
        """`count` or a few more records; in some calls two of them cover the same word (the later wins)."""
        recs = []
        while len(recs) < count:
            first, n = self.voice_range(V, rng)
            r = rng.random()
            if r < 0.55 or not (self.ring_nodes or self.plain_nodes):
                target, node, index, value = self.words[int(rng.integers(0, len(self.words)))]
                recs.append((target, node, index, first, n, value(rng)))
                if rng.random() < 0.3:     # the same word again, over a part of the range: the later record wins
                    recs.append((target, node, index, first + n // 2, n - n // 2, value(rng)))
            elif r < 0.7 and self.sets:
                node = list(self.sets)[int(rng.integers(0, len(self.sets)))]
                col = self.sets[node][:, int(rng.integers(0, 16))]
                recs += [(COEFF, node, i, first, n, _f32(c)) for i, c in enumerate(col)]
            elif self.ring_nodes and (r < 0.88 or not self.plain_nodes):
                recs.append((CLEAR_RINGS, self.ring_nodes[int(rng.integers(0, len(self.ring_nodes)))], 0, first, n, 0))
            else:
                node = self.plain_nodes[int(rng.integers(0, len(self.plain_nodes)))]
                recs.append((CLEAR if (node != -1 or not self.ring_nodes) and rng.random() < 0.8 else CLEAR_RINGS, node, 0, first, n, 0))
        return recs

    def steal(self, v, rng):
        recs = [(CLEAR_RINGS if self.ring_nodes or rng.random() < 0.3 else CLEAR, -1, 0, v, 1, 0)]
        if self.retune:
            target, node, index, value = self.retune[int(rng.integers(0, len(self.retune)))]
            recs.append((target, node, index, v, 1, value(rng)))
        return recs

    def refused(self, V, rng, lists):
        """(call, status name) of a call that must be refused."""
        good = self.records(V, rng, 1)[:1]
        w = self.words[0]
        calls = [(("updates", good + [(w[0], w[1], w[2], V - 1, 2, w[3](rng))]), "ERR_RANGE"),
                 (("updates", good + [(w[0], w[1], w[2], 3, 0, w[3](rng))]), "ERR_INVALID"),
                 (("import_foreign", [0, 1]), "ERR_UNSUPPORTED"), (("import", [4, 9, 4]), "ERR_INVALID"), (("export", [0, V]), "ERR_RANGE")]
        if lists:
            calls += [(("list", [7, 5, 3]), "ERR_INVALID"), (("list", [2, 2]), "ERR_INVALID"), (("list", [0, V]), "ERR_RANGE")]
        calls += [(("updates", good + [(CLEAR, node, 0, 0, 1, 0)]), "ERR_UNSUPPORTED") for node in self.ring_nodes] * 2
        return calls[int(rng.integers(0, len(calls)))]


def make_session(seed, family, lists=True, n_steps=None):
    """The session of (seed, family): types.SimpleNamespace(family, seed, lists, shapes {obj: V}, tables {obj: initial tables}, steps).
    lists=False: no list, listed or steal-into-the-list steps (ring layout 2 has no listed form). Every session begins with a warm-up
    of WARMUP DSPVectors of all voices of both objects (plain steps), compared like every other launch."""
    rng = np.random.default_rng([seed, FAMILIES.index(family), int(lists)])
    VA, VB = shapes(family)
    V = {"A": VA, "B": VB}
    knobs = _Knobs(family)
    cur = {"A": np.zeros(0, np.uint32), "B": np.zeros(0, np.uint32)}
    counter = {"sig": 0, "slot": 0, "launch": 0}
    steps = []

    def sig():
        counter["sig"] += 1
        return seed * 100 + counter["sig"]

    def launch(kind, obj, n):
        counter["launch"] += 1
        st = dict(kind=kind, obj=obj, n=n, sig=sig())
        if kind == "listed":
            st.update(mixdown=family == "bank" and counter["launch"] % 2 == 0, gains=sig())
        return st

    def alive(records, Vo):
        """A bank voice whose frequency is below 2^-64 stands still, and from clear() it is silent: a clear that covers one is followed by
        a phase for it in the same list (the later record wins)."""
        if family != "bank" or seed % 2 == 0:
            return records
        out = list(records)
        for target, node, _, first, n, _ in records:
            if target in (CLEAR, CLEAR_RINGS) and node in (0, -1):
                out += [(STATE, 0, 0, v, 1, int(rng.integers(1 << 28, 1 << 32))) for v in (5, Vo - 3) if first <= v < first + n]
        return out

    for obj in ("A", "B"):
        steps.append(launch("plain", obj, WARMUP))
    # the body: a fixed hand of step kinds in a seeded order, so that a few sessions reach every kind a few times. With lists, a spine on
    # object A keeps its order among the rest: a list, a launch, a list without some of its voices, two launches, a list with them again, a
    # launch - voices come back after launches off the list, in ring layout 4 on a write clock of their own.
    spine = ["list:first", "listed:A", "list:rest", "listed:A", "listed:A", "list:back", "listed:A"] if lists else []
    deck = ["listed", "plain", "updates", "updates", "steal", "move", "move", "refused"] if lists else \
        ["plain"] * 5 + ["updates"] * 3 + ["steal", "move", "move", "move", "refused"]
    deck += [deck[int(rng.integers(0, len(deck)))] for _ in range(int(rng.integers(0, 3)))]
    deck = [deck[j] for j in rng.permutation(len(deck))]
    at = set(rng.choice(len(deck) + len(spine), len(spine), replace=False).tolist()) if spine else set()
    rest, spine_it = iter(deck), iter(spine)
    deck = [next(spine_it) if j in at else next(rest) for j in range(len(deck) + len(spine))]
    if lists:      # the session's first list comes before its first listed launch
        deck.remove("list:first")
        deck.insert(0, "list:first")
    if n_steps:
        deck = deck[:n_steps]
    rested = np.zeros(0, np.uint32)
    since_list = {"A": 0, "B": 0}         # listed launches since the object's list changed
    moved, history = np.zeros(0, np.uint32), {"A": [], "B": []}
    favour, pending = None, []            # the object a move just went into; exports waiting to be put back: (obj, voices, slot, due step)
    for i, kind in enumerate(deck):
        for rec in [r for r in pending if r[3] <= i]:     # put the records back where they came from, some launches later
            pending.remove(rec)
            steps.append(dict(kind="move", op="import", obj=rec[0], voices=rec[1], slot=rec[2]))
        obj = favour if favour and rng.random() < 0.7 else ("A" if rng.random() < 0.7 else "B")
        kind, _, role = kind.partition(":")
        if role:
            obj = "A"
        Vo = V[obj]
        if kind == "list":
            _, L = _draw_list(Vo, rng, LIST_KINDS[seed % len(LIST_KINDS)] if role == "first" else None)     # (the seeds' first lists go through the kinds)
            if role == "rest" and cur[obj].size:
                rested = rng.choice(cur[obj], min(cur[obj].size, int(rng.integers(1, 40))), replace=False).astype(np.uint32)
                L = np.setdiff1d(L, rested).astype(np.uint32)
            elif role == "back":
                L = np.union1d(L, rested).astype(np.uint32)
            elif favour == obj and rng.random() < 0.7:
                L = np.union1d(L, moved).astype(np.uint32)
            elif history[obj] and since_list[obj] >= 2 and rng.random() < 0.7:     # voices of an earlier list come back after launches off the list
                back = np.setdiff1d(history[obj][int(rng.integers(0, len(history[obj])))], cur[obj])
                L = np.union1d(L, back[:int(rng.integers(1, 40))]).astype(np.uint32)
            history[obj].append(L)
            since_list[obj] = 0
            cur[obj] = L
            steps.append(dict(kind="list", obj=obj, L=L))
        elif kind in ("listed", "plain"):
            steps.append(launch(kind, obj, int(rng.integers(1, 4))))
            since_list[obj] += kind == "listed"
            if favour == obj and (kind == "plain" or np.intersect1d(cur[obj], moved).size):
                favour = None
        elif kind == "updates":
            steps.append(dict(kind="updates", obj=obj, records=alive(knobs.records(Vo, rng, int(rng.integers(1, 5))), Vo)))
        elif kind == "steal":
            off = np.setdiff1d(np.arange(Vo), cur[obj])
            v = int(off[int(rng.integers(0, off.size))]) if off.size else int(rng.integers(0, Vo))
            L = np.union1d(cur[obj], [v]).astype(np.uint32) if lists else None
            if lists:
                cur[obj] = L
            steps.append(dict(kind="steal", obj=obj, voice=v, records=alive(knobs.steal(v, rng), Vo), L=L))
        elif kind == "move":
            src = obj
            r = rng.random()
            dst = ("B" if src == "A" else "A") if r < 0.6 else src
            n = int(rng.integers(1, 12))
            if rng.random() < 0.5:
                first, nn = _run_across(V[src], rng, 256)
                S = np.arange(first, first + nn)[:n]
            else:
                S = rng.choice(V[src], n, replace=rng.random() < 0.3)     # export takes repeats
            n = len(S)
            slot = counter["slot"]
            counter["slot"] += 1
            steps.append(dict(kind="move", op="export", obj=src, voices=np.asarray(S, np.uint32), slot=slot))
            if dst == src and r > 0.8 and len(set(S.tolist())) == n:        # aside and back
                pending.append((src, np.asarray(S, np.uint32), slot, i + int(rng.integers(2, 4))))
                continue
            if cur[dst].size >= n and rng.random() < 0.6:      # into listed voices: they sit in wavefronts that are partly listed
                D = rng.choice(cur[dst], n, replace=False)
            else:
                D = rng.choice(V[dst], n, replace=False)
            moved, favour = np.sort(D).astype(np.uint32), dst
            steps.append(dict(kind="move", op="import", obj=dst, voices=np.asarray(D, np.uint32), slot=slot))
        elif kind == "refused":
            call, status = knobs.refused(Vo, rng, lists)
            steps.append(dict(kind="refused", obj=obj, call=call, status=status))
    for rec in pending:
        steps.append(dict(kind="move", op="import", obj=rec[0], voices=rec[1], slot=rec[2]))
    # the drain: what is left in the rings comes out - every delay time at ring length - 64, all voices for ring length / 64 + 1 DSPVectors
    for obj in ("A", "B"):
        drain = [(PARAM, name, 0, 0, V[obj], _f32(DRAIN_DELAY)) for name in ("dt", "dt2") if family in ("string", "three_ring") and (name == "dt" or family == "three_ring")]
        if drain:
            steps.append(dict(kind="updates", obj=obj, records=drain))
        if lists:
            steps.append(dict(kind="list", obj=obj, L=np.arange(V[obj], dtype=np.uint32)))
        steps.append(launch("listed" if lists else "plain", obj, RING // 64 + 1 if knobs.ring_nodes else 2))
        steps[-1]["drain"] = True
    tables = {o: initial_tables(family, V[o], seed + (0 if o == "A" else 5000)) for o in V}
    return types.SimpleNamespace(family=family, seed=seed, lists=lists, shapes=V, tables=tables, steps=steps)


LAYOUTS = {"bank": (0,), "synth": (0,), "string": (0, 1, 4, 2), "three_ring": (0, 1, 4), "pitchbend": (0, 1, 4)}   # ring layouts; 2 has no listed form
DEFAULT_SEEDS = {"bank": 4, "synth": 3}     # every other family: 2 per layout


def default_cases(first=0, count=None, families=FAMILIES):
    """[(family, ring layout, seed, lists)]: the sessions the GPU file runs. The seeds of a (family, layout) are first + 100 * layout +
    0 .. count - 1, so that the layouts of a family walk different sessions. Ring layout 2: sessions without lists, half as many."""
    out = []
    for f in families:
        for layout in LAYOUTS[f]:
            n = count or DEFAULT_SEEDS.get(f, 2)
            if layout == 2:
                n = max(1, n // 2)
            out += [(f, layout, first + 100 * layout + i, layout != 2) for i in range(n)]
    return out


# ---- walking a session through the model --------------------------------------------------------------------------------------------------
def walk_model(session, on_launch=None, worlds=None, on_step=None):
    """The session through session_model alone. Returns (worlds {obj: world}, launches): one entry per launch step, in step order -
    dict(step index, obj, L, n, ys, mix, peaks). on_step(i, step, worlds) is called before each step, on_launch(entry, worlds) after each
    launch."""
    f = session.family
    worlds = worlds or {o: new_world(f, V, session.tables[o]) for o, V in session.shapes.items()}
    cur = {o: np.zeros(0, np.uint32) for o in worlds}
    slots, launches = {}, []
    for i, st in enumerate(session.steps):
        w = worlds[st["obj"]]
        if on_step:
            on_step(i, st, worlds)
        if st["kind"] == "list":
            cur[st["obj"]] = st["L"]
        elif st["kind"] in ("listed", "plain"):
            L = cur[st["obj"]] if st["kind"] == "listed" else np.arange(w.V, dtype=np.uint32)
            if f == "bank":
                mixdown = bool(st.get("mixdown"))
                y, mix, peaks = w.run(L, st["n"], launch_gains(w.V, st["gains"]) if mixdown else None, mixdown)
                entry = dict(step=i, obj=st["obj"], L=L, n=st["n"], ys=[y], mix={} if mix is None else {0: mix}, peaks=peaks)
            else:
                inputs, controls = launch_signals(f, w.V, st["n"], st["sig"], st.get("drain", False))
                ys, mix, peaks = w.run(L, st["n"], inputs, controls)
                entry = dict(step=i, obj=st["obj"], L=L, n=st["n"], ys=ys, mix=mix, peaks=peaks)
            launches.append(entry)
            if on_launch:
                on_launch(entry, worlds)
        elif st["kind"] == "updates":
            w.apply(st["records"])
        elif st["kind"] == "steal":
            w.apply(st["records"])
            if st["L"] is not None:
                cur[st["obj"]] = st["L"]
        elif st["kind"] == "move":
            if st["op"] == "export":
                slots[st["slot"]] = w.take(st["voices"])
            else:
                w.put(st["voices"], slots[st["slot"]])
        elif st["kind"] != "refused":
            raise ValueError(st["kind"])
    return worlds, launches
