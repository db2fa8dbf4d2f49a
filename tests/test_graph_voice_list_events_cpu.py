"""Voice lists for graphs with event rows, without a device (mlgpu_graph_enable_voice_list_events): the listed forms of a kernel with
mlev::CtlVoice - the plain one and the lane plan's -, the plain kernel's source left byte for byte as it is, the refusal that stays
without the switch, the register budget of the instrument bank's listed kernel. Engine-less graphs, as
tests/test_graph_voice_list_cpu.py makes them."""
import re

import pytest

import madronalib_amd as ml
from madronalib_amd import patches
from madronalib_amd.constants import Status
from test_abi import _code_object_notes
from test_graph_voice_list_cpu import refused

V = 2352


def two_node():
    """The two-node event-row graph of the existing refusal tests."""
    return [dict(name="gate", type="event_row", kind=1), dict(name="env", type="proc", kind=ml.Proc.ADSR, inputs=["gate"])], ["env"]


def synth():
    return patches.synth16(pitch_input=True, event_rows=True)


def graph(desc_outputs, V=V, group=0, **switches):
    desc, outputs = desc_outputs
    return ml.Graph(ml.OfflineEngine(), V, desc, outputs, output_groups={0: group} if group else None, compile_now=False, **switches)


GRAPHS = {"two_node": two_node, "synth16": synth}


@pytest.mark.parametrize("which", list(GRAPHS))
def test_emit_listed_with_the_switch(which):
    """The plain listed form: a gfx950 code object whose source has CtlVoice and reads its voice from the list."""
    g = graph(GRAPHS[which](), voice_list_events=True)
    source, code = g.emit_listed()
    assert "mlev::CtlVoice" in source and "a.voiceList[" in source and "a.lanePlan" not in source
    assert ".load(a.events, v_0, a.T)" in source     # the gathered voice, not the lane's place
    assert code[:4] == b"\x7fELF"
    notes = _code_object_notes(code)
    assert "amdgcn-amd-amdhsa--gfx950" in notes and "mlgpu_graph_listed_kernel" in notes
    g.close()


@pytest.mark.parametrize("which", list(GRAPHS))
def test_emit_listed_by_the_lane_plan(which):
    """With the groups switch and a group sum of 16: the lane plan's form."""
    g = graph(GRAPHS[which](), group=16, voice_list_events=True, voice_list_groups=True)
    source, code = g.emit_listed()
    assert "mlev::CtlVoice" in source and "a.lanePlan" in source and "segment_sum_store" in source
    assert ".load(a.events, v_0, a.T)" in source
    assert code[:4] == b"\x7fELF" and "mlgpu_graph_listed_kernel" in _code_object_notes(code)
    g.close()


@pytest.mark.parametrize("which", list(GRAPHS))
@pytest.mark.parametrize("group", [0, 16])
def test_the_plain_source_is_unchanged(which, group):
    """emit()'s source is byte-identical with the switch on and off."""
    on = graph(GRAPHS[which](), group=group, voice_list_events=True, voice_list_groups=bool(group))
    off = graph(GRAPHS[which](), group=group)
    on.emit(), off.emit()
    assert on.source == off.source and "mlev::CtlVoice" in on.source
    assert "voiceList" not in on.source and "lanePlan" not in on.source
    on.close(), off.close()


@pytest.mark.parametrize("which", list(GRAPHS))
@pytest.mark.parametrize("groups", [False, True])
def test_without_the_switch_both_emits_are_refused_as_before(which, groups):
    g = graph(GRAPHS[which](), group=16 if groups else 0, voice_lists=True, voice_list_groups=groups)
    for emit in (g.emit_listed, g.emit):
        refused(Status.ERR_UNSUPPORTED, ["voice lists", "event rows", "go by lane, not by voice: no listed form"], emit)
        assert g.source == "" and g.listed_source() == ""
    g.close()


def test_enable_voice_lists_off_turns_the_switch_off_with_the_rest():
    g = graph(two_node(), voice_list_events=True)
    g.enable_voice_lists(False)
    refused(Status.ERR_INVALID, ["graph_emit_listed", "mlgpu_graph_enable_voice_lists"], g.emit_listed)
    g.enable_voice_lists(True)      # ... and voice lists alone do not bring it back
    refused(Status.ERR_UNSUPPORTED, ["voice lists", "event rows"], g.emit_listed)
    g.close()


def test_the_other_refusals_stay():
    """A mixdown of all voices with the lane plan, and the shard form of a mixdown, are refused with the switch as without."""
    desc, outputs = two_node()
    g = ml.Graph(ml.OfflineEngine(), 2304, desc + [dict(name="half", type="proc", kind=ml.Proc.GAIN, inputs=["env"])], ["env", "half"],
                 output_groups={0: 16}, compile_now=False, voice_list_events=True, voice_list_groups=True)
    g.set_output_mixdown(1, True)
    refused(Status.ERR_UNSUPPORTED, ["voice lists", "mixdown of all voices"], g.emit_listed)
    g.close()
    g = graph(two_node(), V=2304, voice_list_events=True)
    g.set_output_mixdown(0, "shard")
    refused(Status.ERR_UNSUPPORTED, ["voice lists", "shard"], g.emit_listed)
    g.close()


def test_a_mixed_down_output_keeps_the_spare_lanes():
    """A listed graph with event rows and the mixdown of all voices, the bank not a multiple of 64: served with the switch (the spare
    lanes of a last wavefront run the last voice again, event rows included), refused without it as before."""
    g = graph(two_node(), V=120, voice_list_events=True)
    g.set_output_mixdown(0, True)
    source, code = g.emit_listed()
    assert "vr_0 < a.listed ? vr_0 : a.listed - 1" in source and "mix64_park" in source and code[:4] == b"\x7fELF"
    assert g.emit()[1][:4] == b"\x7fELF"
    g.close()
    g = graph(two_node(), V=120)
    g.set_output_mixdown(0, True)
    refused(Status.ERR_UNSUPPORTED, ["event rows", "whole wavefronts"], g.emit)
    g.close()


def test_the_calls_on_a_graph_without_the_switch_name_it():
    g = graph(two_node())
    g.emit()
    for call in (g.process_events_listed, g.process_events_listed_groups):
        refused(Status.ERR_INVALID, ["graph_process_events_listed", "mlgpu_graph_enable_voice_list_events"], call, 1, 0, [], [0], 0, 0, [])
    g.close()


def test_register_budget_of_the_listed_events_kernel(monkeypatch):
    """The listed events kernel of the instrument bank's voice at 262 144 voices, in both listed forms: no private segment where the plain
    fused kernel of the same graph has none (read from the code objects' notes). The VGPR counts are printed."""
    monkeypatch.delenv("MLGPU_GRAPH_MIN_WAVES", raising=False)

    def budget(code):
        notes = _code_object_notes(code)
        return int(re.search(r"\.vgpr_count:\s+(\d+)", notes).group(1)), int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", notes).group(1))
    for groups in (False, True):
        g = graph(synth(), V=262144, group=16 if groups else 0, voice_list_events=True, voice_list_groups=groups)
        plain_vgpr, plain_scratch = budget(g.emit()[1])
        listed_vgpr, listed_scratch = budget(g.emit_listed()[1])
        g.close()
        print(f"synth16 with event rows, V = 262144, {'lane plan' if groups else 'plain list'}: plain kernel {plain_vgpr} VGPRs, {plain_scratch} B "
              f"private; listed kernel {listed_vgpr} VGPRs, {listed_scratch} B private")
        if plain_scratch == 0:
            assert listed_scratch == 0
