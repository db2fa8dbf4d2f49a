"""The SawGen / PulseGen pair on a streamed frequency, without a device: (1) the census - the oracle's own phases and zone tests say
which wave-uniform class every (wavefront, sample) of tests/stream_osc_cases.py's base data falls in, and every class the device code
branches on must be there in numbers, or tests/test_gpu_stream_osc.py would pass without having run that branch; (2) the forms - the
source generated for every structural variant holds the pair form (or does not), which pins planStreamLocks' pairing rules."""
import numpy as np
import pytest

import stream_osc_cases as sc

WAVE_SAMPLE_FLOOR = 200
LANE_SAMPLE_FLOOR = 5000
# the classes step_locked_stream<true / false> and streamLockPair branch on (skip/odd is counted and printed, nothing depends on it)
REQUIRED = ("skip/regular", "single/notfull/regular", "single/notfull/odd", "both/notfull/regular", "both/notfull/odd", "single/full",
            "both/full/regular", "both/full/odd")


@pytest.fixture(scope="module")
def data():
    return sc.census_data()


@pytest.fixture(scope="module")
def cases(data):
    return sc.all_graph_cases(data)


def test_census_reaches_every_class(oracle, data):
    """Measured with the oracle on the committed layout (seed 20240), wave-samples of 64 x 384 per class:
    skip/regular 6103, skip/odd 0, single/notfull/regular 3823, single/notfull/odd 216, both/notfull/regular 6408, both/notfull/odd 1320,
    single/full 1162, both/full/regular 3133, both/full/odd 2411; lane-samples loUp 34916, hiUp 31988, loDown 81727, hiDown 40315.
    The floors (200 wave-samples, 5000 lane-samples) are conditions on the data, not measurements: a class below its floor wants more
    wavefronts of its role in stream_osc_cases.census_data, never a lower floor."""
    classes, zones = sc.census_classes(oracle, data)
    print("census wave-samples:", classes)
    print("census lane-samples:", zones)
    assert sum(classes.values()) == 64 * 64 * 2 * sc.T0
    for k in REQUIRED:
        assert classes[k] >= WAVE_SAMPLE_FLOOR, (k, classes)
    for k, n in zones.items():
        assert n >= LANE_SAMPLE_FLOOR, (k, zones)


def test_census_roles(data):
    """The layout itself: which wavefronts are quiet, which hold only regular widths, where the hostile samples are."""
    wave = sc.wave_of()
    assert data["quiet"].sum() == 16 and (data["f0"][wave < 16] < 0.2 * sc.QUIET * 1.0001).all()
    assert (~data["regular"]).nonzero()[0].tolist() == list(range(48, 60))
    assert data["hostile"][(wave < 32) | (wave >= 48)].sum() == 0 and 0.015 < data["hostile"][(wave >= 32) & (wave < 48)].mean() < 0.025
    w = data["w"][(wave >= 56) & (wave < 60)]
    assert (np.abs(w) <= 1.5).all()                    # mildly odd: the shifted phase stays inside [-2, 2]
    mid = ((wave >= 8) & (wave < 16)) | ((wave >= 24) & (wave < 32))
    assert (data["w"][mid] > 0.1).all() and (data["w"][mid] < 0.9).all()


def offline_graph(case):
    import madronalib_amd as ml
    g = ml.Graph(ml.OfflineEngine(), case.V, case.desc, case.outs, compile_now=False, **case.kwargs)
    for o in case.mix:
        g.set_output_mixdown(o)
    return g


@pytest.mark.parametrize("name", sc.STRUCTURAL + sc.LOCKS)
def test_generated_forms(cases, name):
    """Every variant compiles for gfx950 and its source takes the route the GPU test means to test."""
    case = cases[name]
    g = offline_graph(case)
    source, code = g.emit()
    assert code[:4] == b"\x7fELF"
    sc.assert_forms(case, source)
    ids = g.ids
    pairs, made = sc.lock_table(source)
    vl = 2 if name == "vpl2" else 1
    if name == "signal_width":
        assert pairs == [] and made == []
    elif name not in ("two_pairs_one_freq", "two_freqs"):
        assert pairs == [(ids["saw"], ids["pulse"])] and made == [ids["saw"]]
        assert source.count("step_locked_stream<true>(") == vl and source.count("step_locked_stream<false>(") == vl
        assert source.count("const bool slocked") == 1
    if name == "pulse_first":
        # both values are made where the first of the two stands: before the pulse's own value
        assert ids["pulse"] < ids["saw"]
        at = source.index("step_locked_stream<true>(")
        assert at < source.index(f"const float n{ids['pulse']}_0 = sl{ids['saw']}p_0;") < source.index(f"const float n{ids['saw']}_0 = sl{ids['saw']}s_0;")
    if name == "pair_coeff_w":
        assert f"p{ids['pulse']}_0.next_sw(n{ids['fs']}_0, oddw{ids['pulse']});" in source      # the two-argument fall-back
    if name == "delay_time_from_saw":
        # the delay whose time is made of the saw reads after the pair; the two on parameters read at the top of the sample
        at = source.index("step_locked_stream<true>(")
        assert source.index(f"p{ids['d0']}_0.pre(") > at
        assert source.index(f"p{ids['d1']}_0.pre(") < at and source.index(f"p{ids['d2']}_0.pre(") < at
    g.close()


def test_pairing_rule_as_a_table(cases):
    """planStreamLocks: the first saw on a frequency node takes the first pulse on it (whose width is per voice); nothing else pairs."""
    case = cases["two_pairs_one_freq"]
    g = offline_graph(case)
    source, ids = g.emit()[0], g.ids
    pairs, made = sc.lock_table(source)
    assert pairs == [(ids["saw"], ids["pulse"])] and made == [ids["saw"]]
    assert source.count("const bool slocked") == 1
    assert f"= p{ids['saw2']}_0.next(" in source and f"= p{ids['pulse2']}_0.next_sw(" in source
    assert source.count(f"p{ids['saw']}_0.next(") == 1 and source.count(f"p{ids['pulse']}_0.next_sw(") == 1      # in the fall-back only
    g.close()
    case = cases["two_freqs"]
    g = offline_graph(case)
    source, ids = g.emit()[0], g.ids
    pairs, made = sc.lock_table(source)
    assert pairs == sorted([(ids["saw"], ids["pulse"]), (ids["saw2"], ids["pulse2"])]) and made == sorted([ids["saw"], ids["saw2"]])
    assert source.count("const bool slocked") == 2
    # pulse2 stands before saw2: their pair is made at pulse2's place
    assert source.index(f"float sl{ids['saw']}s") < source.index(f"float sl{ids['saw2']}s") < source.index(f"const float n{ids['pulse2']}_0 = sl{ids['saw2']}p_0;")
    g.close()


@pytest.mark.parametrize("name", sc.LOCKS)
def test_lock_variants_can_tell_a_stale_lock(oracle, cases, name):
    """The lock variants are there for streamLockPair's fall-back, and `slocked` is asked once per launch: a kernel that took an unlocked
    wavefront for locked (a stale `slocked` among them) must leave a trace in what tests/test_gpu_stream_osc.py compares - the pulse's
    output of that launch and its counters after it. Both hypotheses through the oracle: every wavefront whose counters differ when
    a launch begins must differ in at least one compared word of that launch. Measured, output words + counter words that differ, per
    launch: unlock_one_lane 2 + 9 and 1 + 9 (nine wavefronts; a one-unit difference moves the phase by 2^-31 at the most, so the
    counters carry it: the GPU test reads them after every launch), unlock_quarter 78229 + 1024 and 77119 + 1024, relock 122 + 2 in
    launch 2 (the top bit flipped: half a cycle) and no unlocked wavefront in launches 1 and 3; the _oddw forms 2 + 9 and 0 + 9,
    58772 + 1024 and 57727 + 1024, 188 + 2."""
    case = cases[name]
    fell_back, stayed = sc.lock_replay(oracle, case), sc.lock_replay(oracle, case, stay_locked=True)
    seen = 0
    for call, ((a, ca, unlocked), (b, cb, _)) in enumerate(zip(fell_back, stayed)):
        words = ((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).reshape(len(unlocked), -1).sum(1)
        counters = (ca != cb).reshape(len(unlocked), 64).sum(1)
        print(f"{name} launch {call}: {int(unlocked.sum())} unlocked wavefronts, {int(words.sum())} output words and {int(counters.sum())} counter words tell")
        assert ((words + counters)[unlocked] > 0).all(), (name, call, np.flatnonzero(unlocked & (words + counters == 0)))
        assert (words + counters)[~unlocked].sum() == 0
        seen += int(unlocked.sum())
    assert seen > 0
    if name.startswith("relock"):
        assert [int(u.sum()) for _, _, u in fell_back] == [0, 2, 0]
