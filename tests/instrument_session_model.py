"""A host model of an instrument-bank session (TEST INFRASTRUCTURE, no GPU, no HIP): the reference's own EventsToSignals class makes the
event rows, the project's CPU oracle everything downstream of them.

The rows. For every instrument the reference's class (oracle/_ref/libdropin_ref.so: e2s_ref_run, test_gpu_events.ref_run) runs once over
the whole session's events: all V = N P voices' rows per frame; under MPE the reference already adds the main voice's rows.
A launch. The model's description is the device graph's with every event_row node turned into an input node of the same name; a listed
launch of n vectors at start_offset is session_model.GraphWorld.run(L, n, inputs = those rows' frames of the launch), a plain
process_events block is L = arange(V).
Group sums. A group-summed output is accumulated in voice order from +0.0 with the checker's float32 add
(voice_list_groups_cases.expected_listed_groups): one row per listed instrument.
Update records go through GraphWorld.apply; the lists are tails_rule.Rule fed with the model's peaks.

What the model relies on is include/mlgpu.h's own qualification (VOICE LISTS FOR GRAPHS WITH EVENT ROWS, and the MPE section): under drift 0
every row of a listed voice has the bits of the all-voices rows; with drift > 0 a voice's pitch row is exact only if the voice was listed
in every launch since clear - so sessions whose lists change run at drift 0, sessions with drift list every voice in every launch, and
no comparison is left out in either kind."""
import numpy as np

import instrument_session_steps as iss
import tails_rule
from graph_voice_list_cases import expected_peaks
from madronalib_amd.constants import Proc
from session_model import GraphWorld
from voice_list_groups_cases import expected_listed_groups, model_plan, PAD

ADSR_SEGMENT = 7     # oracle/ml_oracle.c: the ADSR's state words are y, y1, x1, threshold, target, k, amp, segment
QUIET_BITS = int(np.float32(iss.QUIET).view(np.uint32))
_rows = {}


class InstrumentWorld(GraphWorld):
    """GraphWorld with the one processor of this graph whose clear() is not a full reset: ADSR::clear() puts the segment to off and
    leaves the envelope's other seven words alone (a CLEAR record is T::clear() of the node for those voices)."""

    def _clear_node(self, name, sl, rings):
        node = self.nodes[name]
        if node["type"] == "proc" and node["kind"] == Proc.ADSR:
            self.st[name][ADSR_SEGMENT, sl] = self.oracle.chain_clear([Proc.ADSR], 1)[ADSR_SEGMENT, 0]
            return
        super()._clear_node(name, sl, rings)


def model_description(desc):
    return [dict(name=n["name"], type="input") if n["type"] == "event_row" else n for n in desc]


def reference_rows(session):
    """[7][V][FRAMES] float32 (read-only): the reference's rows of every voice over the whole session, one run per instrument."""
    key = (session.family, session.seed)
    if key not in _rows:
        from test_gpu_events import ref_run
        refs = [ref_run(session.cfg, evs, iss.BLOCK, iss.N_BLOCKS + 1) for evs in session.instruments]
        rows = np.ascontiguousarray(np.concatenate(refs, 1)[:7])
        rows.setflags(write=False)
        _rows.clear()      # one session's rows at a time
        _rows[key] = rows
    return _rows[key]


def new_world(session, V=None, voices=None):
    """The world after clear() and the session's tables; voices: a world of those voices only."""
    sel = slice(None) if voices is None else np.asarray(voices, np.int64)
    w = InstrumentWorld(iss.oracle(), model_description(session.desc), session.outputs, session.V if voices is None else len(sel), (0,) if session.mix else ())
    w.load({k: a[sel] for k, a in session.params.items()}, {k: a[:, sel] for k, a in session.coeffs.items()})
    return w


def gate_sounding(rows, f0, n):
    """The voices whose reference gate row is non-zero anywhere in the launch: the lower bound of the router's sounding set, and the
    must-set of a walk without a device."""
    return np.flatnonzero(np.any(rows[1][:, f0:f0 + 64 * n] != 0, axis=1)).astype(np.uint32)


def instruments_with_events(session, f0, n):
    return np.array([i for i, evs in enumerate(session.instruments) if any(f0 <= e[3] < f0 + 64 * n for e in evs)], np.int64)


class Walker:
    """The session through the model, launch by launch. launch() returns dict(block, k, n, off, f0, plain, S, L, ys - every output's K
    per-voice rows -, groups {output: J rows}, M - the listed instruments -, mix {output: row}, peaks)."""

    def __init__(self, session):
        self.s, self.rows, self.world = session, reference_rows(session), new_world(session)
        self.rule = tails_rule.Rule(hold=iss.HOLD)
        self.everyone = np.arange(session.V, dtype=np.uint32)

    def begin_block(self, blk):
        self.world.apply(blk["updates"])

    def launch(self, blk, k, sounding=None):
        s, (n, off) = self.s, blk["launches"][k]
        f0 = blk["index"] * iss.BLOCK + off
        S = None
        if blk["plain"]:
            L = self.everyone
        else:
            S = gate_sounding(self.rows, f0, n) if sounding is None else np.asarray(sounding, np.uint32)
            L = self.rule.next_list(self.everyone if s.all_listed else S)
        inputs = {iss.ROW_NAMES[r]: self.rows[r][:, f0:f0 + 64 * n] for r in s.rows}
        ys, mix, peaks = self.world.run(L, n, inputs)
        if not blk["plain"]:
            self.rule.note(n, tails_rule.loud_bits(peaks, QUIET_BITS))
        groups, M = {}, None
        if s.group:
            groups[0], M = expected_listed_groups(self.world.oracle, ys[0], L, s.group)
        return dict(block=blk["index"], k=k, n=n, off=off, f0=f0, plain=blk["plain"], S=S, L=L, ys=ys, groups=groups, M=M, mix=mix, peaks=peaks)


def walk(session):
    """The whole session with the gate rows' sounding sets. Returns (world, launches)."""
    w, out = Walker(session), []
    for blk in session.blocks:
        w.begin_block(blk)
        out += [w.launch(blk, k) for k in range(len(blk["launches"]))]
    return w.world, out


def listed_wavefronts(L, group):
    """The voices of each wavefront of a listed launch: 64 consecutive list positions, or 64 consecutive lanes of the lane plan."""
    lanes = [int(v) for v in L] if not group else model_plan(L, group)[0]
    return [[v for v in lanes[i:i + 64] if v != PAD] for i in range(0, len(lanes), 64)]
