"""Launches in up to four kernels, two per stream (mlgpu_engine_set_launch_parts(3); DESIGN.md §3.1, "Launch parts"): each stream's
window of the bank's voices cut once more computes the bits one launch computes, a call still counts as one launch in parts and the
streams still meet once, and what never went out in parts still does not. T = 3 and the two chains of test_gpu_launch_parts.py;
V = 8448 (2048 + 2048 | 2048 + 2304: four kernels, a ragged last one), 8192 (four whole units), 4096 (a unit a stream: the two halves),
256 (one workgroup: one launch) - the smallest shapes at which a window's offsets, the ragged part and the stream assignment can go
wrong."""
import pytest

from inputs import assert_bits_equal
from madronalib_amd.constants import Layout, Proc
from test_gpu_launch_parts import T, UNIT, expected, make_bank, voice_major

pytestmark = pytest.mark.gpu

QUARTERS = 3
SHAPES = [8448, 8192, 4096, 256]


@pytest.fixture()
def engine():
    """A fresh engine per test (the counters start at zero), parts = 3: two kernels a stream whenever the windows have the units."""
    import madronalib_amd as ml
    e = ml.Engine(0)
    e.set_launch_parts(QUARTERS)
    assert e.get_launch_parts() == QUARTERS
    yield e
    e.close()


@pytest.fixture()
def plain():
    import madronalib_amd as ml
    e = ml.Engine(0)
    e.set_launch_parts(1)
    yield e
    e.close()


@pytest.mark.parametrize("V", SHAPES)
@pytest.mark.parametrize("chain", ["saw", "sine"])
def test_plan_equals_one_launch_equals_the_checker(engine, plain, chain, V):
    """Three consecutive process calls into two alternating buffers: the outputs still there afterwards (calls 2 and 3) and the state
    are the plain engine's bits and the checker's. A call counts once however many kernels it is, nothing joins between the calls,
    and the first download meets the side stream once."""
    want, want_state = expected(chain, V)
    n = V * T * 64
    got = {}
    for eng in (engine, plain):
        in_parts = eng is engine and V > UNIT
        bank = make_bank(eng, chain, V)
        bufs = [eng.alloc(4 * n), eng.alloc(4 * n)]
        eng.sync()
        for k in range(3):
            bank.process(T, bufs[k & 1], Layout.QUAD)
        assert eng.launch_stats() == ((3, 0) if in_parts else (0, 0)), f"V = {V}, parts = {eng.get_launch_parts()}"
        second = voice_major(bufs[1].download(), V)
        assert eng.launch_stats() == ((3, 1) if in_parts else (0, 0))
        got[eng] = (second, voice_major(bufs[0].download(), V), bank.get_all_state())
        assert eng.launch_stats() == ((3, 1) if in_parts else (0, 0))
    label = f"{chain}, V = {V}: "
    for k, (what, ref) in enumerate([("the second call's output", want[1]), ("the third call's output", want[2])]):
        assert_bits_equal(got[engine][k], got[plain][k], what=label + what + " against one launch")
        assert_bits_equal(got[engine][k], ref, what=label + what + " against the checker")
    assert (got[engine][2] == got[plain][2]).all(), label + "the state against one launch"
    assert (got[engine][2] == want_state).all(), label + "the state against the checker"


@pytest.mark.parametrize("layout", [Layout.ROWS, Layout.VOICE_MAJOR])
def test_plan_in_the_other_layouts(engine, layout):
    """Every part's output starts at its first voice in every layout (V = 8448: parts at voices 0, 2048, 4096 and 6144)."""
    V = 8448
    want, _ = expected("saw", V)
    bank = make_bank(engine, "saw", V)
    d_out = engine.alloc(4 * V * T * 64)
    bank.process(T, d_out, layout)
    assert engine.launch_stats() == (1, 0)
    assert_bits_equal(voice_major(d_out.download(), V, layout), want[0], what=f"layout {int(layout)}")
    assert engine.launch_stats() == (1, 1)


def test_what_never_goes_out_in_parts_still_does_not(engine):
    """A streamed-input bank, and any launch while recording a sequence."""
    V = 8448
    n = V * T * 64
    bank = make_bank(engine, "saw", V)
    d_a, d_b = engine.alloc(4 * n), engine.alloc(4 * n)
    flt = engine.bank([Proc.BANDPASS], V)
    flt.process(T, d_b, Layout.QUAD, d_a, Layout.QUAD)
    assert engine.launch_stats() == (0, 0), "a streamed-input bank"
    with engine.record() as seq:
        bank.process(T, d_a, Layout.QUAD)
    assert engine.launch_stats() == (0, 0), "while recording"
    seq.launch()
    engine.sync()
    assert engine.launch_stats() == (0, 0)
    seq.close()


def test_a_mode_there_is_not_is_refused(engine):
    import madronalib_amd as ml
    with pytest.raises(ml.MlgpuError, match="set_launch_parts"):
        engine.set_launch_parts(4)
    assert engine.get_launch_parts() == QUARTERS
