"""Cases for a SawGen / PulseGen pair on a STREAMED frequency (graph_codegen.cpp: planStreamLocks, streamLockPair; mldsp_procs.hpp:
step_locked_stream, Proc<PULSE_GEN>::next_sw / next2) and for the [SAW_GEN] / [PULSE_GEN] banks on the same signal, shared by
tests/test_stream_osc_cpu.py (the census of the wave-uniform classes with the oracle, the generated source's forms) and
tests/test_gpu_stream_osc.py (the device against the oracle, bit for bit). Everything is deterministic from SEED.

The base data ("census"): 4096 voices = 64 wavefronts at one voice per lane, 3 DSPVectors per launch, a frequency that moves every sample,
random 32-bit start counters equal for saw and pulse. Every wave-uniform exit falls back for the whole wavefront when one lane needs it,
so the wavefronts have roles - one class's fall-back cannot hide another class's miss:
  waves  0-15  quiet: the frequency times 0.002, most wave-samples have no lane near a step (the skip exit)
  waves  8-15, 24-31  widths uniform in (0.1, 0.9): no lane is ever inside two zones at once (one shared correction)
  all others   per 16 voices the widths 0, 1, f, 1 - f, f / 2 (f: the voice's base frequency), then uniform in [0, 1]: lanes inside the
               zone of the rising AND of the falling step (two corrections)
  waves 32-47  2 % of the frequency samples replaced by hostile values (`full`: the IEEE division and the reference's operation order)
  waves 48-55  every third voice an absurd width (oddw: step_locked_stream<false>, and `full` through the shifted phase)
  waves 56-59  every third voice a mildly odd width (oddw, the shifted phase stays inside [-2, 2]: step_locked_stream<false>, not `full`)
"""
from collections import namedtuple

import numpy as np

from madronalib_amd.constants import Op, Proc

SEED = 20240
V0, T0 = 4096, 3
MAX_VECTORS = 9          # the longest case: three launches of three DSPVectors
QUIET = 0.002
HOSTILE_FREQS = np.array([0.0, -0.0, -0.01, 1e-25, 1e-38, 1e-45, 1e30, np.inf, -np.inf, np.nan, 0.5, 0.7, 1.5, 2.0 ** -64, 2.0 ** -65,
                          2.0 ** 64, 2.0 ** 65, 1.0], np.float32)
HOSTILE_PITCHES = np.array([np.nan, np.inf, -np.inf, 200.0, -200.0], np.float32)
ABSURD_WIDTHS = np.array([3.0e9, -3.0e9, 2.0 ** 30, -(2.0 ** 30), 2.0 ** 31, np.inf, -np.inf, np.nan, 1.0e20, 1.5, -0.25, 2.0 ** 29], np.float32)
MILD_WIDTHS = np.array([1.5, -0.25, 1.0000001, -1e-9, 1.25, -0.5], np.float32)

# a case: the graph (desc, outs), its per-voice values, {oscillator: start counters}, {input: [V][64 * all vectors]} and the launches -
# [(T, None or what set_state does to the pulse's counters before the launch: apply_launch_edit), ...] - then what the tests need to know
# about it: voices, the strings its generated source must / must not hold, Graph's keyword arguments, the mixed-down outputs' indices,
# the voices that are not quiet
Case = namedtuple("Case", "desc outs params coeffs start_states input_signals launches name V must must_not kwargs mix loud")


def wave_of(V=V0):
    return np.arange(V) // 64


def census_data(seed=SEED):
    """dict: f0 [V] (the base frequency, quiet factor included), f [V][64 MAX_VECTORS] float32, hostile (bool, same shape: the replaced
    samples), w [V], phases [V] uint32, and per wavefront: quiet, regular (every width inside [0, 1])."""
    rng = np.random.default_rng(seed)
    V, S = V0, 64 * MAX_VECTORS
    wave = wave_of(V)
    f0 = np.exp(rng.uniform(np.log(1e-4), np.log(0.2), V))
    f0[wave < 16] *= QUIET
    n, v = np.arange(S)[None, :], np.arange(V)[:, None]
    f = (f0[:, None] * (1.0 + 0.03 * np.sin(2.0 * np.pi * n / 97.0 + 0.37 * v))).astype(np.float32)
    f0 = f0.astype(np.float32)
    hostile = np.zeros((V, S), bool)
    rows = (wave >= 32) & (wave < 48)
    hostile[rows] = rng.random((int(rows.sum()), S)) < 0.02
    pick = rng.integers(0, HOSTILE_FREQS.size, (V, S))
    f[hostile] = HOSTILE_FREQS[pick[hostile]]
    w = rng.uniform(0.0, 1.0, V).astype(np.float32)
    w[0::16], w[1::16] = 0.0, 1.0
    w[2::16] = f0[2::16]
    w[3::16] = np.float32(1.0) - f0[3::16]
    w[4::16] = f0[4::16] * np.float32(0.5)
    mid = ((wave >= 8) & (wave < 16)) | ((wave >= 24) & (wave < 32))
    w[mid] = rng.uniform(0.1, 0.9, int(mid.sum())).astype(np.float32)
    third = np.arange(V) % 3 == 0
    absurd, mild = third & (wave >= 48) & (wave < 56), third & (wave >= 56) & (wave < 60)
    w[absurd] = ABSURD_WIDTHS[rng.integers(0, ABSURD_WIDTHS.size, int(absurd.sum()))]
    w[mild] = MILD_WIDTHS[rng.integers(0, MILD_WIDTHS.size, int(mild.sum()))]
    phases = rng.integers(0, 2 ** 32, V, dtype=np.uint64).astype(np.uint32)
    with np.errstate(invalid="ignore"):
        odd = ~((w >= 0) & (w <= 1))
    return dict(f0=f0, f=np.ascontiguousarray(f), hostile=hostile, w=w, phases=phases, quiet=np.arange(V // 64) < 16,
                regular=~odd.reshape(-1, 64).any(1), seed=seed)


def census_masks(oracle, data, vectors=2 * T0):
    """The wave-uniform classes of every (wavefront, sample) of the census's two launches at one voice per lane, from the ORACLE's
    phases: PhasorGen on the same signal and counters, the shifted phase through the oracle's subtract, add and fractionalPart (float32
    steps as in phasorToPulse), the zone tests against dt = f and 1 - f. -> ({class: [waves][samples] bool}, {zone: [V][samples] bool})."""
    V, S = V0, 64 * vectors
    f, w = np.ascontiguousarray(data["f"][:, :S]), np.ascontiguousarray(np.repeat(data["w"][:, None], S, 1))
    st = np.ascontiguousarray(data["phases"][None, :].copy())
    p = oracle.chain_process([Proc.PHASOR_GEN], vectors, np.zeros((0, V), np.float32), st, f, None)
    one = np.ones((V, S), np.float32)
    d = oracle.op(Op.ADD, oracle.op(Op.SUBTRACT, p, w).view(np.float32), one).view(np.float32)
    down = oracle.op(Op.FRACTIONAL_PART, d).view(np.float32).reshape(V, S)
    omdt = oracle.op(Op.SUBTRACT, one, f).view(np.float32).reshape(V, S)
    with np.errstate(invalid="ignore"):
        loUp, loDown = p < f, down < f
        hiUp, hiDown = ~loUp & (p > omdt), ~loDown & (down > omdt)
        downOdd = ~(np.abs(down) <= 2.0)
    notRegular = (f.view(np.uint32) - np.uint32(0x1F800000)) > np.uint32(0x5F800000 - 0x1F800000)      # blep_freq_not_regular
    nearUp, nearDown = loUp | hiUp, loDown | hiDown
    by_wave = lambda m: m.reshape(V // 64, 64, S).any(1)    # noqa: E731
    regular = data["regular"][:, None]                      # [waves][1]: step_locked_stream<true>, where downOdd is constant false
    near, both = by_wave(nearUp | nearDown), by_wave(nearUp & nearDown)
    full = np.where(regular, by_wave(notRegular), by_wave(notRegular | downOdd))
    single = near & ~both
    classes = {"skip/regular": ~near & regular, "skip/odd": ~near & ~regular,
               "single/notfull/regular": single & ~full & regular, "single/notfull/odd": single & ~full & ~regular,
               "both/notfull/regular": both & ~full & regular, "both/notfull/odd": both & ~full & ~regular,
               "single/full": single & full,
               "both/full/regular": both & full & regular, "both/full/odd": both & full & ~regular}
    return classes, {"loUp": loUp, "hiUp": hiUp, "loDown": loDown, "hiDown": hiDown}


def census_classes(oracle, data, vectors=2 * T0):
    """census_masks counted: ({class: wave-samples}, {zone: lane-samples})."""
    classes, zones = census_masks(oracle, data, vectors)
    return {k: int(m.sum()) for k, m in classes.items()}, {k: int(m.sum()) for k, m in zones.items()}


# ---- the graphs ----------------------------------------------------------------------------------------------------------------

PAIR = ("step_locked_stream<true>(", "step_locked_stream<false>(", "slocked")


def _pair_desc(width="param"):
    d = [dict(name="fs", type="input")]
    if width == "param":
        d += [dict(name="w", type="param")]
    elif width == "voice_op":
        d += [dict(name="wa", type="param"), dict(name="wb", type="param"), dict(name="w", type="op", kind=Op.MULTIPLY, inputs=["wa", "wb"])]
    elif width == "signal":
        d += [dict(name="w", type="input")]
    d += [dict(name="saw", type="proc", kind=Proc.SAW_GEN, inputs=["fs"]),
          dict(name="pulse", type="proc", kind=Proc.PULSE_GEN, inputs=["fs"] if width == "coeff" else ["fs", "w"])]
    return d


def _sel(x, voices):
    return np.ascontiguousarray(x[voices])


def _case(name, desc, outs, data, voices=None, widths=None, launches=None, must=PAIR, must_not=(), oscs=None, kwargs=None, mix=(),
          extra_inputs=None, start=None, **values):
    """Fill in a case from the census data of `voices` (default: all). The width goes wherever the graph wants one: param w, params
    wa * wb, the signal w, the coefficient of every PulseGen without a width input."""
    voices = np.arange(V0) if voices is None else np.asarray(voices)
    V = voices.size
    w = _sel(data["w"] if widths is None else widths, voices)
    names = {d["name"]: d for d in desc}
    launches = launches or [(T0, None), (T0, None)]
    S = 64 * sum(t for t, _ in launches)
    sig = {"fs": np.ascontiguousarray(data["f"][voices, :S])}
    params, coeffs = {}, {}
    if "w" in names and names["w"]["type"] == "param":
        params["w"] = w
    if "wa" in names:   # w = wa * wb exactly: wb a power of two
        params["wa"], params["wb"] = (w * np.float32(4.0)).astype(np.float32), np.full(V, 0.25, np.float32)
    if "w" in names and names["w"]["type"] == "input":
        sig["w"] = np.ascontiguousarray(np.repeat(w[:, None], S, 1))
    for d in desc:
        if d["type"] == "proc" and d["kind"] == Proc.PULSE_GEN and len(d["inputs"]) == 1:
            coeffs[d["name"]] = np.ascontiguousarray(w[None, :])
    for k, x in (extra_inputs or {}).items():
        sig[k] = np.ascontiguousarray(x[voices, :S])
    params.update(values.pop("params", {}))
    oscs = oscs or [d["name"] for d in desc if d["type"] == "proc" and d["kind"] in (Proc.SAW_GEN, Proc.PULSE_GEN)]
    states = {o: _sel(data["phases"], voices).copy() for o in oscs}
    states.update(start or {})
    loud = wave_of(V0)[voices] >= 16
    assert not values, values
    return Case(desc, list(outs), params, coeffs, states, sig, launches, name, V, tuple(must), tuple(must_not), dict(kwargs or {}), tuple(mix), loud)


def rolled_widths(data):
    """The census widths with the odd-width wavefronts 48-59 moved to 20-31 - into the lock variants' unlocked voices."""
    return np.roll(data["w"], -28 * 64)


def structural_cases(data):
    """name -> Case, the structural variants (the census itself is pair_param_w)."""
    c = {}
    sw = ["saw", "pulse"]
    c["pair_param_w"] = _case("pair_param_w", _pair_desc("param"), sw, data, must_not=(".next2(",))
    c["pair_coeff_w"] = _case("pair_coeff_w", _pair_desc("coeff"), sw, data, must=PAIR + ("pulse_width_is_odd(",), must_not=(".next2(",))
    c["pair_voice_op_w"] = _case("pair_voice_op_w", _pair_desc("voice_op"), sw, data, must_not=(".next2(",))
    d = _pair_desc("param")
    c["pulse_first"] = _case("pulse_first", d[:2] + [d[3], d[2]], sw, data, must_not=(".next2(",))
    d = [dict(name="fs", type="input"), dict(name="w", type="param"),
         dict(name="saw", type="proc", kind=Proc.SAW_GEN, inputs=["fs"]), dict(name="saw2", type="proc", kind=Proc.SAW_GEN, inputs=["fs"]),
         dict(name="pulse", type="proc", kind=Proc.PULSE_GEN, inputs=["fs", "w"]), dict(name="pulse2", type="proc", kind=Proc.PULSE_GEN, inputs=["fs"])]
    c["two_pairs_one_freq"] = _case("two_pairs_one_freq", d, ["saw", "saw2", "pulse", "pulse2"], data)
    d = [dict(name="fs", type="input"), dict(name="fs2", type="input"), dict(name="w", type="param"),
         dict(name="saw", type="proc", kind=Proc.SAW_GEN, inputs=["fs"]), dict(name="pulse2", type="proc", kind=Proc.PULSE_GEN, inputs=["fs2"]),
         dict(name="saw2", type="proc", kind=Proc.SAW_GEN, inputs=["fs2"]), dict(name="pulse", type="proc", kind=Proc.PULSE_GEN, inputs=["fs", "w"])]
    # the second frequency: the census's a fifth higher, on the voices of the wavefront 17 further on (every role meets every other)
    f2 = (np.roll(data["f"], 17 * 64, axis=0) * np.float32(1.5)).astype(np.float32)
    c["two_freqs"] = _case("two_freqs", d, ["saw", "pulse", "saw2", "pulse2"], data, extra_inputs={"fs2": f2})
    c["signal_width"] = _case("signal_width", _pair_desc("signal"), sw, data, must=(".next2(", ".next("), must_not=("step_locked_stream", "slocked"))
    # fs = exp2Approx(pitch) * base inside the graph (patches.synth16): base the voice's own frequency, the pitch the sweep in octaves;
    # the hostile samples go in through the pitch
    S = data["f"].shape[1]
    n, v = np.arange(S)[None, :], np.arange(V0)[:, None]
    pitch = np.log2(1.0 + 0.03 * np.sin(2.0 * np.pi * n / 97.0 + 0.37 * v)).astype(np.float32)
    pick = np.random.default_rng(data["seed"] + 1).integers(0, HOSTILE_PITCHES.size, pitch.shape)
    pitch[data["hostile"]] = HOSTILE_PITCHES[pick[data["hostile"]]]
    d = [dict(name="fs", type="input"), dict(name="pitch", type="input"), dict(name="base", type="param"), dict(name="w", type="param"),
         dict(name="ratio", type="op", kind=Op.EXP2_APPROX, inputs=["pitch"]), dict(name="freq", type="op", kind=Op.MULTIPLY, inputs=["ratio", "base"]),
         dict(name="saw", type="proc", kind=Proc.SAW_GEN, inputs=["freq"]), dict(name="pulse", type="proc", kind=Proc.PULSE_GEN, inputs=["freq", "w"])]
    c["computed_freq"] = _case("computed_freq", d[1:], sw, data, extra_inputs={"pitch": pitch}, params={"base": data["f0"]}, must_not=(".next2(",))
    c["computed_freq"].input_signals.pop("fs")
    # two voices per lane: the census twice, the second copy on other counters
    two = np.concatenate([np.arange(V0), np.arange(V0)])
    other = np.random.default_rng(data["seed"] + 2).integers(0, 2 ** 32, V0, dtype=np.uint64).astype(np.uint32)
    ph2 = np.concatenate([data["phases"], other])
    c["vpl2"] = _case("vpl2", _pair_desc("param"), sw, data, voices=two, kwargs=dict(voices_per_lane=2), start={"saw": ph2.copy(), "pulse": ph2.copy()},
                      must=PAIR + ("(2 voice",), must_not=(".next2(",))
    # nine workgroups and a last wavefront of 6 voices: a quiet half, both width roles, five wavefronts and the ragged one with hostile frequencies
    c["ragged"] = _case("ragged", _pair_desc("param"), sw, data, voices=np.arange(2374), must_not=(".next2(",))
    d = _pair_desc("param") + [dict(name="sum", type="op", kind=Op.ADD, inputs=["saw", "pulse"])]
    c["ragged_mix"] = _case("ragged_mix", d, sw + ["sum"], data, voices=np.arange(2374), mix=(2,), must=PAIR + ("ldsMix",), must_not=(".next2(",))
    # ring layout 0 with early reads (three rings): one delay time made of the saw, which is made with its partner where the first of
    # the two stands and cannot go to the top of the sample; the loud wavefronts 16-23 (edge widths, no hostile values: a NaN delay time
    # is another test's business)
    d = _pair_desc("param") + [dict(name="dt1", type="param"), dict(name="dt2", type="param"), dict(name="c40", type="const", value=40.0),
                               dict(name="c39", type="const", value=39.0),
                               dict(name="sa", type="op", kind=Op.ABS, inputs=["saw"]), dict(name="ss", type="op", kind=Op.MULTIPLY, inputs=["sa", "c40"]),
                               dict(name="dl", type="op", kind=Op.MIN, inputs=["ss", "c39"]),
                               dict(name="d0", type="proc", kind=Proc.INTEGER_DELAY, inputs=["pulse", "dl"], max_delay=40.0),
                               dict(name="d1", type="proc", kind=Proc.INTEGER_DELAY, inputs=["saw", "dt1"], max_delay=40.0),
                               dict(name="d2", type="proc", kind=Proc.INTEGER_DELAY, inputs=["pulse", "dt2"], max_delay=40.0)]
    vo = np.arange(1024, 1536)
    c["delay_time_from_saw"] = _case("delay_time_from_saw", d, sw + ["d0", "d1", "d2"], data, voices=vo, launches=[(4, None), (4, None)],
                                     params={"dt1": ((np.arange(512) * 7) % 40).astype(np.float32), "dt2": ((np.arange(512) * 13) % 37).astype(np.float32)},
                                     must=PAIR + ("ldsEarly",), must_not=(".next2(",), oscs=["saw", "pulse"], kwargs=dict(delay_windows=0))
    return c


def lock_cases(data):
    """name -> Case: pair_param_w with counters that differ, on the census widths and (`_oddw`) with the odd-width wavefronts inside
    the unlocked voices, so that the fall-back runs next_sw with oddW false and true."""
    c = {}
    rng = np.random.default_rng(data["seed"] + 3)
    V = V0
    for tag, widths in (("", None), ("_oddw", rolled_widths(data))):
        ph = data["phases"]
        one = ph.copy()
        one[64 * 5 + 3::64 * 7] ^= np.uint32(1)         # wavefronts 5, 12, 19, 26, ... 61
        c["unlock_one_lane" + tag] = _case("unlock_one_lane" + tag, _pair_desc("param"), ["saw", "pulse"], data, widths=widths, start={"pulse": one})
        quarter = ph.copy()
        quarter[V // 4:V // 2] = rng.integers(0, 2 ** 32, V // 4, dtype=np.uint64).astype(np.uint32)
        c["unlock_quarter" + tag] = _case("unlock_quarter" + tag, _pair_desc("param"), ["saw", "pulse"], data, widths=widths, start={"pulse": quarter})
        # launch 1 locked; before launch 2 one lane's pulse counter flipped in wavefronts 5 and 26 (its top bit, half a cycle: a launch 2
        # that stayed locked shows in that lane's output, and in its counter after the launch, which the test reads before the next edit);
        # before launch 3 the pulse's counters set to the saw's again
        c["relock" + tag] = _case("relock" + tag, _pair_desc("param"), ["saw", "pulse"], data, widths=widths,
                                  launches=[(T0, None), (T0, ("flip", [64 * 5 + 3, 64 * 26 + 40])), (T0, ("equal", None))])
    return c


def all_graph_cases(data):
    c = structural_cases(data)
    c.update(lock_cases(data))
    return c


STRUCTURAL = ("pair_param_w", "pair_coeff_w", "pair_voice_op_w", "pulse_first", "two_pairs_one_freq", "two_freqs", "signal_width", "computed_freq",
              "vpl2", "ragged", "ragged_mix", "delay_time_from_saw")
LOCKS = tuple(n + t for t in ("", "_oddw") for n in ("unlock_one_lane", "unlock_quarter", "relock"))


def assert_forms(case, source):
    """The strings a case's generated source must and must not hold."""
    for s in case.must:
        assert s in source, (case.name, "missing", s)
    for s in case.must_not:
        assert s not in source, (case.name, "unexpected", s)


def lock_table(source):
    """The pairs in a generated source: [(saw node, pulse node)] from `slocked<i> = ... p<i>.omega32 != p<j>.omega32`, and the nodes
    whose values are made as a pair (sl<i>s / sl<i>p declarations)."""
    import re
    pairs = sorted({(int(a), int(b)) for a, b in re.findall(r"const bool slocked(\d+) = [^;]*?p\1(?:_\d+)?\.omega32 != p(\d+)(?:_\d+)?\.omega32", source)})
    made = sorted({int(a) for a in re.findall(r"float sl(\d+)s(?:_\d+)?, sl\1p", source)})
    return pairs, made


def apply_launch_edit(edit, saw_counters, pulse_counters):
    """The pulse's counters a launch's edit asks for, given both oscillators' counters at that moment."""
    kind, lanes = edit
    out = saw_counters.copy() if kind == "equal" else pulse_counters.copy()
    if kind == "flip":
        out[lanes] ^= np.uint32(0x80000000)
    return out


def lock_replay(oracle, case, stay_locked=False):
    """A lock case through the oracle, launch by launch: [(pulse output [V][64 T], pulse counters after the launch, the wavefronts whose
    counters differed when the launch began)]. stay_locked: what a kernel would compute that took every wavefront for locked - the
    pulse's counters made the saw's when the launch begins (step_locked_stream writes pulse.omega32 = saw.omega32)."""
    from graph_oracle import evaluate
    V = case.V
    states = {d["name"]: oracle.chain_clear([d["kind"]], V) for d in case.desc if d["type"] == "proc"}
    for o, ph in case.start_states.items():
        states[o][0] = ph
    at, res = 0, []
    for T, edit in case.launches:
        if edit is not None:
            states["pulse"][0] = apply_launch_edit(edit, states["saw"][0], states["pulse"][0])
        unlocked = (states["saw"][0] != states["pulse"][0]).reshape(-1, 64).any(1)
        if stay_locked:
            states["pulse"][0] = states["saw"][0]
        sig = {k: np.ascontiguousarray(x[:, at:at + 64 * T]) for k, x in case.input_signals.items()}
        at += 64 * T
        out = evaluate(oracle, case.desc, ["pulse"], V, T, sig, case.params, case.coeffs, states)[0]
        res.append((out, states["pulse"][0].copy(), unlocked))
    return res


def freq_of(oracle, case):
    """[V][S] the frequency the case's `saw` sees, by the oracle: the input itself or the ops it is made of."""
    from graph_oracle import evaluate
    node = next(d for d in case.desc if d["name"] == "saw")["inputs"][0]
    k = next(i for i, d in enumerate(case.desc) if d["name"] == node)
    sub = [d for d in case.desc[:k + 1] if d["type"] != "proc"]
    T = sum(t for t, _ in case.launches)
    return evaluate(oracle, sub, [node], case.V, T, case.input_signals, case.params, {}, {})[0]


def bank_case(data, kind):
    """(procs, coeffs [NC][V], start state [1][V], signal [V][64 * 2 T0]) of the [SAW_GEN] / [PULSE_GEN] bank on the census's signal;
    the pulse's width is the processor's coefficient."""
    co = np.ascontiguousarray(data["w"][None, :]) if kind == Proc.PULSE_GEN else np.zeros((0, V0), np.float32)
    return [kind], co, np.ascontiguousarray(data["phases"][None, :].copy()), np.ascontiguousarray(data["f"][:, :64 * 2 * T0])
