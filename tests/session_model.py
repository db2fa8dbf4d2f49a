"""A host model of a whole session of a live voice bank (TEST INFRASTRUCTURE, no GPU, no HIP): everything that is per voice, for all V
voices of a graph or of a fused bank, and the calls that change it - listed and plain launches, update records, voice records.

The one rule (include/mlgpu.h, VOICE LISTS): a listed call behaves exactly as an object of K voices made of L[0] ... L[K-1], and nobody
else is touched. So a launch gathers the listed voices' tables, state, ring memory and input rows, runs the project's CPU oracle
(cpu_checkers.Oracle through graph_oracle.evaluate_stream / evaluate, or oracle.chain_process) on those K voices, and scatters the state
back. Update records and voice records follow the header word by word: records are applied one at a time in list order, CLEAR is
T::clear() of the node for those voices, CLEAR_RINGS that plus zeros to the node's rings (the write index stays), a voice record is an
exact image of every per-voice word. tests/test_session_model_cpu.py checks the model against V independent one-voice models.

Records are plain data, (target, node, index, first_voice, n_voices, bits): `target` one of the names below, `node` a graph's node
NAME or a bank's processor index (-1: every processor and feedback node)."""
import types

import numpy as np

import graph_oracle
import graph_voice_list_cases as gcases
import voice_list_cases as bcases
from madronalib_amd.constants import Proc

PARAM, COEFF, STATE, INPUT_CONST, CLEAR, CLEAR_RINGS = "param", "coeff", "state", "input_const", "clear", "clear_rings"
RING_WRITE_INDEX_WORDS = {Proc.INTEGER_DELAY: (0,), Proc.FRACTIONAL_DELAY: (0,), Proc.PITCHBENDABLE_DELAY: (0, 5)}   # oracle/ml_oracle.c, delay lines
_cleared_words = {}


def cleared_words(oracle, kind, max_delay=100.0):
    """{state word: value after T::clear()} of one processor kind, taken through the oracle. A processor without rings: every word,
    at the oracle's state after clear(). A delay node: clear() is a std::fill of the ring and the clear() of its allpass section, so it
    resets the filter memories and leaves alone the write index and the delay-time words a setter wrote - the words that keep
    changing while the node runs on a CONSTANT delay time (a state after one DSPVector against the state after two), less the write
    indices."""
    kind = int(kind)
    if kind in _cleared_words:
        return _cleared_words[kind]
    after_clear = oracle.chain_clear([kind], 1)[:, 0]
    if kind not in Proc.DELAYS:
        words = {i: int(w) for i, w in enumerate(after_clear)}
    else:
        from inputs import lcg_noise
        st = oracle.chain_default_state([kind], 1)
        rings = 2 if kind == Proc.PITCHBENDABLE_DELAY else 1
        mem = np.zeros((1, rings, graph_oracle.ring_len(max_delay)), np.float32)
        x, dt = lcg_noise(np.array([7], np.uint32), 128), np.full((1, 128), 9.37, np.float32)
        oracle.delay_process(kind, 1, st, mem, [x[:, :64], dt[:, :64]])
        one = st.copy()
        oracle.delay_process(kind, 1, st, mem, [x[:, 64:], dt[:, 64:]])
        moving = np.flatnonzero((one != st).any(1))
        words = {int(i): int(after_clear[i]) for i in moving if int(i) not in RING_WRITE_INDEX_WORDS[kind]}
    _cleared_words[kind] = words
    return words


def _rows(a):
    return np.ascontiguousarray(a)


class GraphWorld:
    """Everything per voice of a compiled graph after clear(): params {name: [V]}, coeffs {name: [NC][V]}, and graph_oracle's stream state -
    proc state {name: [NS][V] uint32}, rings {name + "/mem": [V][rings][len]}, feedback vectors {name: [V][64]}."""

    def __init__(self, oracle, desc, outputs, V, mix=()):
        self.oracle, self.desc, self.outputs, self.V, self.mix = oracle, desc, list(outputs), int(V), tuple(mix)
        self.nodes = {n["name"]: n for n in desc}
        self.params = {n["name"]: np.zeros(V, np.float32) for n in desc if n["type"] == "param"}
        self.coeffs = {n["name"]: np.zeros((oracle.num_coeffs(n["kind"]), V), np.float32) for n in desc
                       if n["type"] == "proc" and oracle.num_coeffs(n["kind"]) > 0}
        self.st = graph_oracle.new_stream_state(oracle, desc, V)
        for n in desc:
            if n["type"] == "proc":
                self.st[n["name"]] = oracle.chain_clear([n["kind"]], V)
        self.streamed = any(n["type"] == "feedback" or (n["type"] == "proc" and n["kind"] in Proc.DELAYS) for n in desc)
        self.state_nodes = [n["name"] for n in desc if n["type"] in ("proc", "feedback")]

    # ---- where a voice's words live: proc state is [NS][V], rings and feedback vectors are [V][...] ---------------------------------
    def _voice_axis(self, key):
        return 1 if (key in self.nodes and self.nodes[key]["type"] == "proc") else 0

    def load(self, params=None, coeffs=None, states=None):
        for k, a in (params or {}).items():
            self.params[k][:] = a
        for k, a in (coeffs or {}).items():
            self.coeffs[k][:] = a
        for k, a in (states or {}).items():
            self.st[k][:] = a

    def state_row(self, name, i):
        """State word i of a node as the getters give it: [V] uint32 (a feedback node's word i is sample i of its stored vector)."""
        a = self.st[name]
        return a[i].copy() if self._voice_axis(name) == 1 else np.ascontiguousarray(a[:, i]).view(np.uint32).copy()

    def num_state(self, name):
        a = self.st[name]
        return a.shape[0] if self._voice_axis(name) == 1 else a.shape[1]

    # ---- launches ----------------------------------------------------------------------------------------------------------------------
    def run(self, L, n, inputs, controls=None):
        """A launch of n DSPVectors of the voices L (ascending): inputs {name: [V][64 n]}, controls {name: [V][n]} keep their V rows.
        Returns (outputs [K][64 n] each, {output index: mixed-down row [64 n]}, peaks [K] uint32)."""
        L = np.asarray(L, np.int64)
        K, controls = L.size, controls or {}
        if K == 0:
            ys = [np.zeros((0, 64 * n), np.float32) for _ in self.outputs]
            return ys, {o: np.zeros(64 * n, np.float32) for o in self.mix}, np.zeros(0, np.uint32)
        sig = {k: _rows(np.asarray(a, np.float32)[L]) for k, a in inputs.items()}
        sig.update({k: _rows(np.asarray(a, np.float32)[L]) for k, a in controls.items()})
        params = {k: _rows(a[L]) for k, a in self.params.items()}
        coeffs = {k: _rows(a[:, L]) for k, a in self.coeffs.items()}
        st = {k: _rows(np.take(a, L, self._voice_axis(k))) for k, a in self.st.items()}
        fn = graph_oracle.evaluate_stream if self.streamed else graph_oracle.evaluate
        ys = [np.ascontiguousarray(y, np.float32) for y in fn(self.oracle, self.desc, self.outputs, K, n, sig, params, coeffs, st)]
        for k, a in self.st.items():
            if self._voice_axis(k) == 1:
                a[:, L] = st[k]
            else:
                a[L] = st[k]
        return ys, {o: gcases.expected_mixdown(self.oracle, ys[o]) for o in self.mix}, gcases.expected_peaks(ys)

    # ---- update records ----------------------------------------------------------------------------------------------------------------
    def _clear_node(self, name, sl, rings):
        node = self.nodes[name]
        if node["type"] == "feedback":
            self.st[name][sl] = 0.0
            return
        for i, value in cleared_words(self.oracle, node["kind"]).items():
            self.st[name][i, sl] = np.uint32(value)
        if rings and name + "/mem" in self.st:
            self.st[name + "/mem"][sl] = 0.0

    def apply(self, records):
        for target, node, index, first, n, bits in records:
            assert 0 < n and first + n <= self.V
            sl, word = slice(first, first + n), np.uint32(bits)
            if target == PARAM:
                self.params[node].view(np.uint32)[sl] = word
            elif target == COEFF:
                self.coeffs[node].view(np.uint32)[index, sl] = word
            elif target == STATE:
                if self._voice_axis(node) == 1:
                    self.st[node][index, sl] = word
                else:
                    self.st[node].view(np.uint32)[sl, index] = word
            elif target in (CLEAR, CLEAR_RINGS):
                for name in (self.state_nodes if node == -1 else [node]):
                    assert target == CLEAR_RINGS or name + "/mem" not in self.st, "CLEAR of a node with rings is refused"
                    self._clear_node(name, sl, target == CLEAR_RINGS)
            else:
                raise ValueError(target)

    # ---- voice records -----------------------------------------------------------------------------------------------------------------
    def take(self, voices):
        """One exact image per entry of `voices` (any order, repeats allowed)."""
        out = []
        for v in np.asarray(voices, np.int64):
            out.append(dict(params={k: a[v].copy() for k, a in self.params.items()}, coeffs={k: a[:, v].copy() for k, a in self.coeffs.items()},
                            st={k: np.take(a, v, self._voice_axis(k)).copy() for k, a in self.st.items()}))
        return out

    def put(self, voices, slices):
        voices = np.asarray(voices, np.int64)
        assert len(set(voices.tolist())) == voices.size == len(slices), "import wants distinct voices"
        for v, s in zip(voices, slices):
            for k, a in self.params.items():
                a[v] = s["params"][k]
            for k, a in self.coeffs.items():
                a[:, v] = s["coeffs"][k]
            for k, a in self.st.items():
                if self._voice_axis(k) == 1:
                    a[:, v] = s["st"][k]
                else:
                    a[v] = s["st"][k]

    # ---- read-backs --------------------------------------------------------------------------------------------------------------------
    def tables(self):
        """{("param", name, 0) | ("coeff", name, i) | ("state", name, i): [V] uint32}: every row the getters read."""
        t = {("param", k, 0): a.view(np.uint32).copy() for k, a in self.params.items()}
        for k, a in self.coeffs.items():
            for i in range(a.shape[0]):
                t[("coeff", k, i)] = a[i].view(np.uint32).copy()
        for k in self.state_nodes:
            for i in range(self.num_state(k)):
                t[("state", k, i)] = self.state_row(k, i)
        return t

    def record_table_words(self, v):
        """The table words of voice v's record in the documented order: every params row, every coefficient row, every state row
        (feedback vectors included), rows in node order."""
        t = self.tables()
        keys = [k for kind in ("param", "coeff", "state") for n in self.desc for k in t if k[0] == kind and k[1] == n["name"]]
        return np.array([t[k][v] for k in keys], np.uint32)


class BankWorld:
    """Everything per voice of a fused bank after clear(): coeffs [NC][V], state [NS][V] uint32 (both in chain order), the input const."""

    def __init__(self, oracle, procs, V):
        self.oracle, self.procs, self.V = oracle, [int(p) for p in procs], int(V)
        nc, _ = oracle.chain_sizes(self.procs)
        self.coeffs = np.zeros((nc, V), np.float32)
        self.state = oracle.chain_clear(self.procs, V)
        self.in_const = np.zeros(V, np.float32)
        self.c0 = np.cumsum([0] + [oracle.num_coeffs(p) for p in self.procs])
        self.s0 = np.cumsum([0] + [oracle.num_state(p) for p in self.procs])

    def load(self, coeffs, in_const, state=None):
        self.coeffs[:], self.in_const[:] = coeffs, in_const
        if state is not None:
            self.state[:] = state

    def _chain(self):
        return types.SimpleNamespace(procs=self.procs, coeffs=self.coeffs, in_const=self.in_const, in_rows=None, in_group=1)

    def run(self, L, n, gains=None, mixdown=False):
        """A launch of n DSPVectors of the voices L. Returns (y [K][64 n], the mixed-down row [64 n] or None, peaks [K] uint32);
        gains [V] go by voice."""
        L = np.asarray(L, np.int64)
        y = bcases.expected_listed(self.oracle, self._chain(), L, self.state, 0, n)
        mix = bcases.expected_listed_mixdown(self.oracle, y, L, gains) if mixdown else None
        return y, mix, bcases.expected_peaks(y)

    def apply(self, records):
        for target, node, index, first, n, bits in records:
            assert 0 < n and first + n <= self.V
            sl, word = slice(first, first + n), np.uint32(bits)
            if target == COEFF:
                self.coeffs.view(np.uint32)[self.c0[node] + index, sl] = word
            elif target == STATE:
                self.state[self.s0[node] + index, sl] = word
            elif target == INPUT_CONST:
                self.in_const.view(np.uint32)[sl] = word
            elif target in (CLEAR, CLEAR_RINGS):   # banks have no rings: exactly CLEAR
                for p in (range(len(self.procs)) if node == -1 else [node]):
                    for i, value in cleared_words(self.oracle, self.procs[p]).items():
                        self.state[self.s0[p] + i, sl] = np.uint32(value)
            else:
                raise ValueError(target)

    def take(self, voices):
        return [dict(coeffs=self.coeffs[:, v].copy(), state=self.state[:, v].copy(), in_const=self.in_const[v].copy()) for v in np.asarray(voices, np.int64)]

    def put(self, voices, slices):
        voices = np.asarray(voices, np.int64)
        assert len(set(voices.tolist())) == voices.size == len(slices), "import wants distinct voices"
        for v, s in zip(voices, slices):
            self.coeffs[:, v], self.state[:, v], self.in_const[v] = s["coeffs"], s["state"], s["in_const"]

    def tables(self):
        t = {}
        for p in range(len(self.procs)):
            for i in range(self.c0[p + 1] - self.c0[p]):
                t[("coeff", p, i)] = self.coeffs[self.c0[p] + i].view(np.uint32).copy()
            for i in range(self.s0[p + 1] - self.s0[p]):
                t[("state", p, i)] = self.state[self.s0[p] + i].copy()
        t[("input_const", 0, 0)] = self.in_const.view(np.uint32).copy()
        return t

    def record_table_words(self, v):
        """Voice v's record: every coefficient row, every state row, the input-const word (zeros up to a multiple of 4 follow)."""
        return np.concatenate([self.coeffs[:, v].view(np.uint32), self.state[:, v], self.in_const[v:v + 1].view(np.uint32)]).astype(np.uint32)
