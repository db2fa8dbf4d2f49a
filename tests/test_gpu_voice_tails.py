"""Voice tails on the device (mlgpu_tails_*, madronalib_amd.VoiceTails): the loud bits voice_tails_kernel makes of a launch's peaks,
the hold, results that are still out when the next list is made, and the intended block end to end on a fused bank and on an events
graph. Expected values: numpy on the peaks and tests/tails_rule.py, the header's rule restated over Python sets. Every comparison is
on integers."""
import numpy as np
import pytest

import tails_rule

pytestmark = pytest.mark.gpu
Q = int(np.float32(1e-4).view(np.uint32))


@pytest.fixture(scope="module")
def eng():
    import madronalib_amd as ml
    e = ml.Engine(0)
    yield e
    e.close()


def quiet_float(bits):
    return np.uint32(bits).view(np.float32)


def same(a, b):
    return np.array_equal(np.asarray(a, np.uint32), np.asarray(b, np.uint32))


@pytest.mark.parametrize("K", [0, 1, 63, 64, 65, 257])
def test_loud_bits(eng, K):
    """Synthetic peaks around the threshold, infinity's and a NaN's bits, and random words; a list of stride-3 voices of 1 024. The first
    launch resets every voice (all are in its must-set); after the second, next_list([]) with hold 1 is exactly the voices numpy
    finds above the threshold. K = 0 enqueues nothing and has nothing pending."""
    import madronalib_amd as ml
    tails = ml.VoiceTails(eng, 1024, 512, depth=2)
    tails.set_threshold(quiet_float(Q), 1)
    voices = (3 * np.arange(K)).astype(np.uint32)
    special = np.array([0, Q - 1, Q, Q + 1, 0x7F800000, 0x7FC00000, 0xFFFFFFFF, 1], np.uint32)
    peaks = np.random.default_rng(K).integers(0, 2 ** 31, K + 1, dtype=np.uint64).astype(np.uint32)
    peaks[1::2] = (peaks[1::2] % np.uint32(2 * Q)).astype(np.uint32)      # half of the random ones around the threshold
    n = min(K, special.size)
    peaks[:n] = special[:n]
    if K > 64:
        peaks[K - special.size:K] = special                                # ... and at the list's end, across a word's end where there is one
    peaks[K] = 0xFFFFFFFF                                                  # the word behind the K peaks is nobody's
    d_peak = eng.to_device(peaks)
    assert same(tails.next_list(voices), voices)
    tails.note(1, d_peak)
    assert tails.pending == (1 if K else 0)
    tails.wait()
    assert tails.pending == 0
    assert same(tails.next_list([]), voices)
    tails.note(1, d_peak)
    tails.wait()
    want = voices[tails_rule.loud_bits(peaks[:K], Q)]
    got = tails.next_list([])
    assert same(got, want), (got, want)
    if K >= 6:
        assert 3 * 3 in want and 3 * 4 in want and 3 * 5 in want and 3 * 2 not in want and 0 not in want
    tails.close()


def test_hold_over_launches_of_1_and_3_vectors(eng):
    """hold_vectors = 4: a voice leaves at the launch that reaches the hold; a loud launch and a must-set reset it."""
    import madronalib_amd as ml
    tails = ml.VoiceTails(eng, 64, 16, depth=2)
    tails.set_threshold(quiet_float(Q), 4)
    rule = tails_rule.Rule(hold=4)
    d_peak = eng.alloc(64)
    q, loud = 5, Q + 1

    def block(must, want, vectors, peaks):
        got = tails.next_list(must)
        assert same(got, want) and same(rule.next_list(must), want), (got, want)
        if peaks is not None:
            d_peak.upload(np.array(peaks + [0xFFFFFFFF], np.uint32))
            tails.note(vectors, d_peak)
            rule.note(vectors, tails_rule.loud_bits(peaks, Q))
            tails.wait()
    block([3, 9, 20], [3, 9, 20], 1, [q, q, q])        # all in the must-set: 0, 0, 0
    block([], [3, 9, 20], 3, [q, q, q])                # 3, 3, 3
    block([], [3, 9, 20], 1, [q, loud, q])             # 4, 0, 4
    block([20], [9, 20], 3, [q, q])                    # voice 3 left at the launch that reached 4; 20 is back by the must-set: 9: 3, 20: 0
    block([], [9, 20], 1, [q, q])                      # 4, 1
    block([], [20], 3, [q])                            # 4
    block([], [], None, None)
    with pytest.raises(ml.MlgpuError) as ei:
        tails.set_threshold(quiet_float(Q), 0)
    assert ei.value.status == ml.Status.ERR_INVALID
    tails.close()


def test_two_results_out_and_no_wait(eng):
    """Two launches noted, next_list at once: whatever has arrived, the list is the rule's with 0, 1 or 2 results taken in - a superset of
    the rule's given both - and after wait() the next list is the rule's given everything."""
    import madronalib_amd as ml
    V, K = 1024, 300
    rng = np.random.default_rng(7)
    tails = ml.VoiceTails(eng, V, 512, depth=4)
    tails.set_threshold(quiet_float(Q), 1)
    A = np.sort(rng.choice(V, K, replace=False)).astype(np.uint32)
    B = A[::5].copy()

    def peaks_for(L):
        p = rng.integers(0, 2 * Q, len(L) + 1, dtype=np.uint64).astype(np.uint32)
        return p[:-1], eng.to_device(p)
    L1 = tails.next_list(A)
    p1, d1 = peaks_for(L1)
    tails.note(1, d1)
    L2 = tails.next_list(B)
    p2, d2 = peaks_for(L2)
    tails.note(2, d2)
    L3 = tails.next_list([])           # no wait, no sync: the device is where it is
    assert same(L1, A) and same(L2, A)
    candidates = []
    for c in (0, 1, 2):
        r = tails_rule.Rule(hold=1)
        r.next_list(A)
        r.note(1, tails_rule.loud_bits(p1, Q))
        r.next_list(B, taken_in=0)
        r.note(2, tails_rule.loud_bits(p2, Q))
        candidates.append((r, r.next_list([], taken_in=c)))
    assert len(candidates[2][1]) < len(candidates[1][1]) == len(candidates[0][1]) == K
    taken = [c for c in (0, 1, 2) if same(candidates[c][1], L3)]
    assert taken, "the list is none of the rule's three"
    assert np.all(np.isin(candidates[2][1], L3))
    rule = candidates[taken[0]][0]
    p3, d3 = peaks_for(L3)
    tails.note(1, d3)
    rule.note(1, tails_rule.loud_bits(p3, Q))
    assert 1 <= tails.pending <= 3
    tails.wait()
    assert tails.pending == 0
    got = tails.next_list([])
    assert same(got, rule.next_list([])) and 0 < len(got) < len(L3)
    tails.close()


def test_end_to_end_on_a_fused_bank(eng):
    """128 Bandpass voices of different damping on a streamed input that is loud for every third voice in the first block and zero
    afterwards; 40 blocks of next_list -> set_voice_list -> process_listed(d_peak) -> note, the engine synchronised before each
    next_list. The lists are the rule's on the downloaded peaks, block by block; every voice that left had hold_vectors quiet
    DSPVectors behind it; silent voices leave first, ringing ones as they decay."""
    import madronalib_amd as ml
    from inputs import lcg_noise
    from madronalib_amd.constants import Layout, Proc
    V, T, HOLD = 128, 1, 3
    bank = eng.bank([Proc.BANDPASS], V)
    assert bank.fused
    bank.clear()
    k = 0.02 + 0.5 * (np.arange(V) % 16) / 16.0
    bank.set_all_coeffs(np.ascontiguousarray(np.stack([ml.Bandpass.makeCoeffs(0.05 + 0.001 * v, float(k[v])) for v in range(V)], 1)))
    bank.reserve_voice_list(V)
    x = lcg_noise(np.arange(V, dtype=np.uint32) + 29, 64 * T)
    x[np.arange(V) % 3 != 0] = 0.0
    d_x, d_zero = eng.to_device(x), eng.to_device(np.zeros_like(x))
    d_out, d_peak = eng.alloc(4 * V * 64 * T), eng.alloc(4 * V + 4)
    tails = ml.VoiceTails(eng, V, V, depth=4)
    tails.set_threshold(1e-4, HOLD)
    rule = tails_rule.Rule(hold=HOLD)
    sizes = []
    for b in range(40):
        must = np.arange(V, dtype=np.uint32) if b == 0 else np.zeros(0, np.uint32)
        eng.sync()
        L = tails.next_list(must)
        assert same(L, rule.next_list(must)), f"block {b}"
        sizes.append(len(L))
        bank.set_voice_list(L)
        bank.process_listed(T, d_out, Layout.QUAD, d_x if b == 0 else d_zero, Layout.VOICE_MAJOR, d_peak)
        tails.note(T, d_peak)
        peaks = d_peak.download(np.uint32, max(len(L), 1))[:len(L)]
        rule.note(T, tails_rule.loud_bits(peaks, Q))
    assert sizes[0] == V and sizes[HOLD] == V and sizes[HOLD + 1] <= V - 85       # the silent voices: listed HOLD launches after their must-set
    assert sizes[-1] < sizes[HOLD + 1] and len(set(sizes)) > 4, sizes            # the ringing ones go one after the other
    assert len(rule.quiet_behind) >= 85 and min(rule.quiet_behind.values()) >= HOLD
    tails.close(), bank.close()


def test_end_to_end_through_the_intended_block(eng):
    """16 instruments x 4 voices: gate row -> ADSR x sine at the pitch row, summed per instrument, listed by the lane plan with event
    rows. A short performance of note-ons, note-offs and a retrigger through add_events -> route_ahead -> sounding_graph_voices ->
    next_list -> set_voice_list -> process_events_listed_groups(d_peak) -> note -> clear_events. Every list holds the sounding voices;
    a released voice stays until its recorded peaks show the hold and is gone the block after (the lists are the rule's)."""
    import madronalib_amd as ml
    from madronalib_amd.constants import Layout, Op, Proc
    N, P, T, HOLD = 16, 4, 2, 4
    V = N * P
    ev = ml.Events(eng, N, P, 48000.0)
    ev.configure(glide_seconds=0.0, drift=0.0)
    ev.set_wanted_rows([0, 1])
    desc = [dict(name="gate", type="event_row", kind=1), dict(name="pitch", type="event_row", kind=0), dict(name="baseFreq", type="param"),
            dict(name="ratio", type="op", kind=Op.EXP2_APPROX, inputs=["pitch"]),
            dict(name="freq", type="op", kind=Op.MULTIPLY, inputs=["ratio", "baseFreq"]),
            dict(name="osc", type="proc", kind=Proc.SINE_GEN, inputs=["freq"]),
            dict(name="env", type="proc", kind=Proc.ADSR, inputs=["gate"]),
            dict(name="out", type="op", kind=Op.MULTIPLY, inputs=["osc", "env"])]
    g = ml.Graph(eng, V, desc, ["out"], output_groups={0: P}, voice_lists=True, voice_list_groups=True, voice_list_events=True)
    g.clear()
    g.set_param("baseFreq", 440.0 / 48000.0)
    g.set_coeffs("env", [np.full(V, c, np.float32) for c in ml.ADSR.calcCoeffs(0.001, 0.01, 0.7, 0.03, 48000.0)])   # a release of some 550 samples, four launches, that ends in exact zeros
    g.bind_events(ev)
    ev.reserve_for_graph(T)
    g.reserve_voice_list_groups(V)
    d_out, d_peak = eng.alloc(4 * N * T * 64), eng.alloc(4 * V + 4)
    tails = ml.VoiceTails(eng, V, V, depth=4)
    tails.set_threshold(1e-4, HOLD)
    rule = tails_rule.Rule(hold=HOLD)
    # (block, instrument, type, key, time): instruments 0 .. 7 play a note in block 1 + i % 3 and release it six blocks later; instrument
    # 2 plays the same key again while its first note is still dying away
    events = []
    for i in range(8):
        events += [(1 + i % 3, i, 1, 60 + i, 7 * i), (7 + i % 3, i, 4, 60 + i, 11)]
    events += [(13, 2, 1, 62, 3), (20, 2, 4, 62, 40)]
    history, sounding_sizes = [], []
    for b in range(40):
        now = [e for e in events if e[0] == b]
        ev.add_events([e[1] for e in now], [ml.Event(e[2], 1, e[3], e[4], (e[3] - 60) / 12.0 if e[2] == 1 else 0.0, 0.8 if e[2] == 1 else 0.0) for e in now])
        ev.route_ahead(T, 0)
        S = ev.sounding_graph_voices()
        eng.sync()
        L = tails.next_list(S)
        assert np.all(np.isin(S, L)), f"block {b}: a sounding voice is not listed"
        assert same(L, rule.next_list(S)), f"block {b}"
        g.set_voice_list(L)
        g.process_events_listed_groups(T, 0, [], [d_out], out_layout=Layout.VOICE_MAJOR, d_peak=d_peak)
        tails.note(T, d_peak)
        peaks = d_peak.download(np.uint32, max(len(L), 1))[:len(L)]
        rule.note(T, tails_rule.loud_bits(peaks, Q))
        ev.clear_events()
        history.append((S, L, peaks))
        sounding_sizes.append(len(S))
    assert max(sounding_sizes) >= 8 and sounding_sizes[-1] == 0
    assert max(int(p.max()) for _, _, p in history if len(p)) > Q, "nothing sounded"
    # tails there were: voices listed though no longer sounding, and loud there; and in the end everybody has left
    assert any(np.any(p[~np.isin(L, S)] > Q) for S, L, p in history if len(L))
    assert len(history[-1][1]) == 0
    # every voice that left: its last HOLD DSPVectors on the list were quiet, it was in no must-set there, and it is gone the block after
    left = 0
    for b in range(1, 40):
        gone = np.setdiff1d(history[b - 1][1], history[b][1])
        for v in gone:
            quiet = 0
            for S, L, p in reversed(history[:b]):
                if v not in L or v in S or p[np.searchsorted(L, v)] > Q:
                    break
                quiet += T
            assert quiet >= HOLD and quiet - T < HOLD, f"voice {v} left at block {b} with {quiet} quiet DSPVectors behind it"
            left += 1
    assert left >= 8        # eight notes (the retrigger's voice may be one of them, still listed)
    tails.close(), g.close(), ev.close()
