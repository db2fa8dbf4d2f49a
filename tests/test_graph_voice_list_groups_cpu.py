"""A graph's listed group sums, without a device: the lane-plan form of the listed kernel (mlgpu_graph_enable_voice_list_groups,
mlgpu_graph_emit_listed), both existing kernels' text left as it is without the switch, and the refusals planGraph decides.
Engine-less graphs throughout."""
import pytest

import madronalib_amd as ml
from graph_voice_list_cases import build_graph, gain_desc, string_desc, synth_desc, three_ring_desc, upsample_graph
from graph_voice_list_groups_cases import GROUPS, V, build_group_graph, offline_case
from madronalib_amd.constants import Proc, Region, Status
from test_abi import _code_object_notes


def offline(desc_outputs, sums, switch=True, voice_lists=False, delay_windows=False, n_voices=V, groups=None):
    return build_group_graph(ml.OfflineEngine(), offline_case(desc_outputs, groups), sums, n_voices, switch, voice_lists, delay_windows)


def refused(status, words, fn, *args):
    with pytest.raises(ml.MlgpuError) as ei:
        fn(*args)
    assert ei.value.status == status, str(ei.value)
    assert all(w in str(ei.value) for w in words), str(ei.value)


@pytest.mark.parametrize("G", GROUPS)
def test_emit_listed_gives_the_lane_plan_form_for_gfx950(G):
    """The synth voice, output 0 summed by G, output 1 plain: the listed kernel finds its voice in the lane plan, sums through the
    segment strip whatever G is - no lane shifts, no 16-voice strip, no voice list - and compiles for gfx950 under the listed name."""
    g = offline(synth_desc(), {0: G})
    source, code = g.emit_listed()
    assert "mlgpu_graph_listed_kernel" in source and "lanePlan" in source and "segment_sum_store" in source and "segment_park" in source
    assert "group16_" not in source and "group_sum_in_order" not in source and "voiceList[" not in source
    assert "trip_locked" in source and "a.peaks[pl_0]" in source and "plan.z" in source
    # a pad leaves before the first wave-uniform ballot, and nothing but the plan entry is loaded before it does
    head = source[:source.index("__builtin_amdgcn_ballot_w64")]
    assert "if (vr_0 >= a.listed) return;" in head and "if (plan.x == 0xFFFFFFFFu) return;" in head and "__syncthreads" not in source
    assert code[:4] == b"\x7fELF"
    notes = _code_object_notes(code)
    assert "amdgcn-amd-amdhsa--gfx950" in notes and "mlgpu_graph_listed_kernel" in notes
    assert g.listed_source() == source
    g.close()


def _numbers(code):
    import re
    notes = _code_object_notes(code)
    return {k: int(re.search(r"\.%s:\s+(\d+)" % k, notes).group(1)) for k in ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}


def test_the_lane_plan_form_keeps_its_voice_in_registers():
    """The synth voice: no scratch, the segment strips' 16 KiB + 256 B of LDS, four wavefronts per SIMD. The config-5 voice over a bank
    big enough for the register budget to apply: the form takes no bound that costs it scratch - its segment sums hold up to 32
    registers of LDS reads next to the voice's state, inside the loop."""
    from madronalib_amd import patches
    g = offline(synth_desc(), {0: 16})
    n = _numbers(g.emit_listed()[1])
    g.close()
    assert n["private_segment_fixed_size"] == 0 and n["group_segment_fixed_size"] == 4 * 4096 + 256 and n["vgpr_count"] <= 128, n
    g = offline(patches.synth16(), {0: 16}, n_voices=262144)
    n = _numbers(g.emit_listed()[1])
    g.close()
    assert n["private_segment_fixed_size"] == 0 and n["group_segment_fixed_size"] == 4 * 4096 + 256, n


def test_the_impulse_table_barrier_comes_before_any_lane_leaves():
    desc = [dict(name="x", type="input"), dict(name="imp", type="proc", kind=Proc.IMPULSE_GEN, inputs=["x"])]
    g = offline((desc, ["imp"]), {0: 4})
    source, code = g.emit_listed()
    assert code[:4] == b"\x7fELF" and source.count("__syncthreads()") == 1
    assert source.index("__syncthreads()") < source.index("return;")
    g.close()


@pytest.mark.parametrize("G", [4, 16])
def test_the_plain_source_is_unchanged(G):
    """The kernel of mlgpu_graph_process of a graph with a group sum: the same text with the switch as without."""
    on, off = offline(synth_desc(), {0: G}), offline(synth_desc(), {0: G}, switch=False)
    on.emit(), off.emit()
    assert on.source == off.source and len(on.source) > 1000
    assert "lanePlan" not in on.source and "segment_" not in on.source
    assert on.listed_source() and off.listed_source() == ""
    on.close(), off.close()


@pytest.mark.parametrize("which", ["synth", "string", "three", "upsample", "gain"])
def test_the_listed_source_without_the_switch_has_no_lane_plan(which):
    """Every graph of graph_voice_list_cases: mlgpu_graph_enable_voice_lists alone makes the listed kernel it made before."""
    if which == "upsample":
        g = upsample_graph(ml.OfflineEngine(), V)
    else:
        desc, mix = {"synth": (synth_desc(), (1,)), "string": (string_desc(), ()), "three": (three_ring_desc(), ()), "gain": (gain_desc(), ())}[which]
        g = build_graph(ml.OfflineEngine(), offline_case(desc), V)
        for o in mix:
            g.set_output_mixdown(o, True)
    source, code = g.emit_listed()
    assert code[:4] == b"\x7fELF" and "a.voiceList[" in source
    assert "lanePlan" not in source and "segment_" not in source
    g.close()


def test_the_switches():
    """enable_voice_list_groups(1) turns voice lists on; enable_voice_lists(0) turns both off; enable_voice_list_groups(0) leaves the
    plain listed form."""
    g = offline(synth_desc(), {})
    g.enable_voice_lists(False)
    refused(Status.ERR_INVALID, ["graph_emit_listed", "mlgpu_graph_enable_voice_lists"], g.emit_listed)
    assert g.emit()[1][:4] == b"\x7fELF" and g.listed_source() == ""
    g.enable_voice_list_groups(True)
    g.enable_voice_list_groups(False)
    source, _ = g.emit_listed()
    assert "a.voiceList[" in source and "lanePlan" not in source
    g.close()


def _mixdown(form):
    def make(switch):
        g = offline(synth_desc(), {0: 16}, switch, n_voices=2304)     # (the shard form wants whole 64-voice groups)
        g.set_output_mixdown(1, form)
        return g
    return make


def _event_rows(switch):
    desc = [dict(name="gate", type="event_row", kind=1), dict(name="env", type="proc", kind=ml.Proc.ADSR, inputs=["gate"])]
    return offline((desc, ["env"]), {0: 16}, switch)


def _downsample(switch):
    g = upsample_graph(ml.OfflineEngine(), V, False, Region.DOWNSAMPLE_2X)
    g.set_output_group_sum(0, 16)
    if switch:
        g.enable_voice_list_groups()
    return g


# (2304 voices for the ring layouts: layout 2 next to a group sum wants whole wavefronts whatever the listed form)
REFUSALS = {
    "no_group_sum": (lambda sw: offline(synth_desc(), {}, sw), Status.ERR_INVALID, ["no output has a group sum", "mlgpu_graph_set_output_group_sum"]),
    "two_group_sizes": (lambda sw: offline(synth_desc(), {0: 16, 1: 4}, sw), Status.ERR_INVALID, ["of 16 and of 4 voices", "one size"]),
    "mixdown": (_mixdown(True), Status.ERR_UNSUPPORTED, ["mixdown of all voices", "pads"]),
    "mixdown_shard": (_mixdown("shard"), Status.ERR_UNSUPPORTED, ["mixdown of all voices", "pads"]),
    "layout1": (lambda sw: offline(string_desc(), {0: 16}, sw, delay_windows=1, n_voices=2304), Status.ERR_UNSUPPORTED, ["delay layout 1", "mlgpu_graph_set_delay_layout(g, 0)"]),
    "layout2": (lambda sw: offline(string_desc(), {0: 16}, sw, delay_windows=2, n_voices=2304), Status.ERR_UNSUPPORTED, ["delay layout 2", "mlgpu_graph_set_delay_layout(g, 0)"]),
    "layout4": (lambda sw: offline(string_desc(), {0: 16}, sw, delay_windows=4, n_voices=2304), Status.ERR_UNSUPPORTED, ["delay layout 4", "mlgpu_graph_set_delay_layout(g, 0)"]),
    "event_rows": (_event_rows, Status.ERR_UNSUPPORTED, ["event rows"]),
    "downsample": (_downsample, Status.ERR_UNSUPPORTED, ["DOWNSAMPLE_2X"]),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_graphs_the_lane_plan_form_does_not_serve_are_refused_at_emit(name):
    """From both emits, with the reason and the switch's name in the message and nothing built; the same graph without the switch
    still emits."""
    make, status, words = REFUSALS[name]
    g = make(True)
    for emit in (g.emit_listed, g.emit):
        refused(status, ["voice lists", "mlgpu_graph_enable_voice_list_groups"] + words, emit)
        assert g.source == "" and g.listed_source() == ""
    g.close()
    g = make(False)
    source, code = g.emit()
    assert code[:4] == b"\x7fELF"
    g.close()


def test_without_the_switch_voice_lists_and_a_group_sum_are_still_refused():
    """... and the message now names the call that serves the pair."""
    g = offline(synth_desc(), {0: 16}, switch=False, voice_lists=True)
    for emit in (g.emit_listed, g.emit):
        refused(Status.ERR_UNSUPPORTED, ["voice lists", "group sum", "mlgpu_graph_enable_voice_list_groups"], emit)
        assert g.source == "" and g.listed_source() == ""
    g.close()


def test_more_lds_than_a_workgroup_has_is_refused_with_the_sizes():
    """Eight outputs summed by 4 (8 x (16 KiB + 256 B) of segment strips) next to the landing slots of 31 early ring reads (31 KiB):
    161 KiB. The plain kernel of the same graph has no strip at all and emits."""
    desc = [dict(name="x", type="input"), dict(name="dt", type="param")]
    for i in range(31):
        desc.append(dict(name=f"d{i}", type="proc", kind=Proc.INTEGER_DELAY, inputs=[f"d{i - 1}" if i else "x", "dt"], max_delay=10.0))
    outputs = [f"d{i}" for i in range(23, 31)]
    g = offline((desc, outputs), {o: 4 for o in range(8)})
    for emit in (g.emit_listed, g.emit):
        refused(Status.ERR_UNSUPPORTED, ["voice lists", "mlgpu_graph_enable_voice_list_groups", "130 KiB", "8 group-summed outputs", "31 KiB", "160 KiB"], emit)
        assert g.source == "" and g.listed_source() == ""
    g.close()
    g = offline((desc, outputs[:7]), {o: 4 for o in range(7)})      # (seven: 145 KiB)
    source, code = g.emit_listed()
    assert code[:4] == b"\x7fELF" and source.count("kSegmentStrip + kSegmentTail") == 7 and "ldsEarly" in source
    g.close()


@pytest.mark.parametrize("rings", [1, 3])
def test_ring_layout_0_and_an_input_group_are_served(rings):
    g = offline(string_desc() if rings == 1 else three_ring_desc(), {0: 16}, groups={"x": 16})
    source, code = g.emit_listed()
    assert code[:4] == b"\x7fELF" and "lanePlan" in source and "(v_0 / 16)" in source
    assert ("ldsEarly" in source) == (rings == 3)
    g.close()


def test_calls_on_a_graph_made_without_the_switch_say_so():
    g = offline(synth_desc(), {}, switch=False, voice_lists=True)
    g.emit()
    refused(Status.ERR_INVALID, ["graph_reserve_voice_list_groups", "mlgpu_graph_enable_voice_list_groups", "before compile"], g.reserve_voice_list_groups, 8)
    refused(Status.ERR_INVALID, ["graph_process_listed_groups", "mlgpu_graph_enable_voice_list_groups", "before compile"], g.process_listed_groups, 1, [0], [0, 0], 0, 0, [0])
    assert g.listed_groups.size == 0
    g.close()
