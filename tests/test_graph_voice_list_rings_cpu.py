"""Voice lists for graphs with sector delay rings (mlgpu_graph_enable_voice_list_rings), without a device: the listed form of a ring
graph in ring layouts 1 and 4, what layout 3 resolves to under the switch, the refusals planGraph decides, and the plain kernel's
source left as it is. Engine-less graphs, as tests/test_graph_voice_list_cpu.py makes them."""
import re

import pytest

import madronalib_amd as ml
from graph_voice_list_cases import build_graph, string_desc, synth_desc, three_ring_desc
from madronalib_amd.constants import Proc, Status
from test_graph_voice_list_cpu import V, case_of, refused

LANE_CLOCK = "#define MLGPU_RING_LANE_CLOCK"


def layout_of(source):
    """The ring layout a generated kernel uses (what layout 3 resolved to): Graph.delay_layout says so after a compile, which needs a
    device (tests/test_gpu_graph_voice_list_rings.py); before one it is the layout asked for, and the source carries the plan's."""
    m = re.search(r"^#define MLGPU_RING_WINDOWS (\d)$", source, re.M)
    return {None: 0, "1": 1, "2": 2, "3": 4}[m and m.group(1)]


DESCS = {"string": string_desc, "three": three_ring_desc}


def offline(desc_outputs, layout, rings=True, voice_lists=True, mix=()):
    g = build_graph(ml.OfflineEngine(), case_of(desc_outputs, mix), V, voice_lists, layout)
    if rings:
        g.enable_voice_list_rings()
    return g


@pytest.mark.parametrize("layout", [1, 4, 3])
@pytest.mark.parametrize("which", ["string", "three"])
def test_emit_listed_under_the_switch(which, layout):
    """The listed kernel of a ring graph in the sector layouts: it reads its voice from the list, keeps the layout's ring windows, and -
    in layout 4 only - runs its trips on each lane's write clock. Layout 3 resolves to 4 for both graphs (their LDS fits, no delay line
    in a rate region) and never to 2."""
    g = offline(DESCS[which](), layout)
    source, code = g.emit_listed()
    resolved = 4 if layout == 3 else layout
    # (before a compile delay_layout is the layout asked for - tests/test_abi.py pins that after an emit of layout 3 -, so the resolved
    # layout is read from the source here and from delay_layout in tests/test_gpu_graph_voice_list_rings.py)
    assert g.delay_layout == layout and layout_of(source) == resolved != 2
    assert code[:4] == b"\x7fELF"
    assert "mlgpu_graph_listed_kernel" in source and "a.voiceList[" in source
    assert f"#define MLGPU_RING_WINDOWS {3 if resolved == 4 else 1}\n" in source and "ldsRings" in source
    assert (LANE_CLOCK in source) == (resolved == 4)
    assert ("trip_begin()" in source) == (resolved == 4)
    plain, plain_code = g.emit()
    assert plain_code[:4] == b"\x7fELF" and layout_of(plain) == resolved and LANE_CLOCK not in plain and "voiceList" not in plain
    g.close()


def test_the_switch_turns_voice_lists_on_and_goes_off_with_them():
    g = offline(string_desc(), 4, voice_lists=False)
    assert g.emit_listed()[1][:4] == b"\x7fELF"
    g.enable_voice_lists(False)
    g.emit()
    assert g.listed_source() == ""
    g.enable_voice_lists(True)    # ... the rings switch went off with the rest: today's refusal, in today's words
    refused(Status.ERR_UNSUPPORTED, ["voice lists", "delay layout 4", "mlgpu_graph_set_delay_layout(g, 0)"], g.emit_listed)
    g.close()


def test_layout_2_stays_refused_with_the_new_words():
    g = offline(string_desc(), 2)
    for emit in (g.emit_listed, g.emit):
        refused(Status.ERR_UNSUPPORTED, ["voice lists", "delay layout 2", "neighbouring lanes", "mlgpu_graph_enable_voice_list_rings", "layouts 1 and 4", "layout 3"], emit)
        assert g.source == "" and g.listed_source() == ""
    g.close()


def test_the_switch_on_a_graph_without_rings_is_invalid():
    g = offline(synth_desc(), False, mix=(1,))
    for emit in (g.emit_listed, g.emit):
        refused(Status.ERR_INVALID, ["mlgpu_graph_enable_voice_list_rings", "no delay node"], emit)
    g.close()


@pytest.mark.parametrize("layout", [1, 4])
@pytest.mark.parametrize("which", ["string", "three"])
def test_the_plain_source_is_unchanged(which, layout):
    """The kernel of mlgpu_graph_process in layouts 1 and 4: the same text with voice lists off and with the rings switch on."""
    on, off = offline(DESCS[which](), layout), offline(DESCS[which](), layout, rings=False, voice_lists=False)
    on.emit(), off.emit()
    assert on.source == off.source and len(on.source) > 1000
    assert on.listed_source() and off.listed_source() == ""
    on.close(), off.close()


def test_the_switch_composes_with_the_lane_plan():
    """Group sums by the lane plan next to rings in layout 1 and 4: the planned kernel has the segment strips and the ring windows."""
    for layout in (1, 4, 3):
        g = offline(string_desc(), layout)
        g.set_output_group_sum(0, 16)
        g.enable_voice_list_groups()
        source, code = g.emit_listed()
        assert code[:4] == b"\x7fELF" and "a.lanePlan" in source and "ldsSeg0" in source and "ldsRings" in source
        assert layout_of(source) == layout_of(g.emit()[0]) == (4 if layout == 3 else layout)
        g.close()


def _delay_bank(n, layout):
    """n FractionalDelays in series on one input: 8 KiB of layout-1 windows each, 24 KiB of layout-4 strips each."""
    desc = [dict(name="x", type="input")]
    for i in range(n):
        desc.append(dict(name=f"d{i}", type="proc", kind=Proc.FRACTIONAL_DELAY, inputs=[desc[-1]["name"]], max_delay=100.0))
    return offline((desc, [f"d{n - 1}"]), layout)


def test_layout_3_falls_back_where_the_lds_does_not_fit():
    """160 KiB of LDS: seven delay nodes want 168 KiB in layout 4 and 56 KiB in layout 1 - layout 3 takes 1; twenty-one want 168 KiB
    in layout 1 too - the rows. Layout 4 asked for by name is refused with the sizes."""
    g = _delay_bank(7, 3)
    assert "a.voiceList[" in g.emit_listed()[0] and layout_of(g.listed_source()) == layout_of(g.source) == 1
    g.close()
    g = _delay_bank(21, 3)
    assert layout_of(g.emit()[0]) == layout_of(g.listed_source()) == 0 and "a.voiceList[" in g.listed_source()
    g.close()
    g = _delay_bank(7, 4)
    refused(Status.ERR_UNSUPPORTED, ["delay layout 4", "168 KiB", "160 KiB"], g.emit)
    g.close()


def test_a_graph_made_without_the_switch_answers_as_before():
    g = offline(string_desc(), 0, rings=False)
    assert g.emit_listed()[1][:4] == b"\x7fELF" and layout_of(g.listed_source()) == 0
    g.close()
    g = offline(string_desc(), 3, rings=False)
    refused(Status.ERR_UNSUPPORTED, ["voice lists", "delay layout 2", "layout 3 resolves", "mlgpu_graph_set_delay_layout(g, 0)"], g.emit_listed)
    g.close()


def test_the_lane_plan_counts_the_ring_windows_in_its_lds():
    """Five delay nodes (120 KiB of layout-4 strips) and three outputs summed by 8 voices: the plain kernel has no LDS beside the rings,
    the lane plan's kernel three segment strips (16 KiB + 256 B each) - 169 KiB. Layout 4 by name is refused with the sizes; layout 3
    takes layout 1 for both kernels."""
    def make(layout):
        desc = [dict(name="x", type="input")]
        for i in range(5):
            desc.append(dict(name=f"d{i}", type="proc", kind=Proc.FRACTIONAL_DELAY, inputs=[desc[-1]["name"]], max_delay=100.0))
        g = offline((desc, ["d4", "d3", "d2"]), layout)
        for o in range(3):
            g.set_output_group_sum(o, 8)
        g.enable_voice_list_groups()
        return g
    g = make(4)
    refused(Status.ERR_UNSUPPORTED, ["mlgpu_graph_enable_voice_list_groups", "mlgpu_graph_enable_voice_list_rings", "120 KiB", "delay layout 4", "49 KiB", "160 KiB"], g.emit)
    g.close()
    g = make(3)
    assert layout_of(g.emit()[0]) == layout_of(g.listed_source()) == 1 and "a.lanePlan" in g.listed_source()
    g.close()


def test_the_strict_aligned_test_is_a_test_hook(monkeypatch):
    """MLGPU_GRAPH_RING_LANE_CLOCK=0: the listed kernel of layout 4 without the macro - the plain kernel's aligned test - and nothing else
    changed; the GPU tests and tools/graph_voice_list_rings_bench.py compare the two."""
    relaxed, strict = offline(string_desc(), 4), offline(string_desc(), 4)
    a = relaxed.emit_listed()[0]
    monkeypatch.setenv("MLGPU_GRAPH_RING_LANE_CLOCK", "0")    # (the hooks are read at every planning)
    b = strict.emit_listed()[0]
    assert LANE_CLOCK in a and LANE_CLOCK not in b and a.replace(LANE_CLOCK + " 1\n", "") == b
    assert "#define MLGPU_RING_BY_LANE 1\n" in a and "#define MLGPU_RING_BY_LANE 1\n" in b and "MLGPU_RING_BY_LANE" not in relaxed.source
    assert relaxed.source == strict.source
    relaxed.close(), strict.close()
