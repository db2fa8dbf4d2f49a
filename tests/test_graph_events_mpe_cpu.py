"""The build switch mlgpu_graph_enable_mpe_events without a device: without it no form's source names the MPE-capable structs
(mlev::CtlVoiceMpe / mlev::CtlRowsMpe), with it the plain form's does and compiles for gfx950 while the listed forms keep their text;
the register budget of the instrument bank's voice with the switch; the refusals that need no device. Engine-less graphs, as
tests/test_graph_event_rows_cpu.py makes them."""
import re

import pytest

import madronalib_amd as ml
from madronalib_amd import patches
from madronalib_amd.constants import Status
from test_abi import _code_object_notes, _header
from test_graph_event_rows_cpu import graph, rows_desc, three_forms
from test_graph_voice_list_cpu import refused

# What the switched kernel may keep in scratch beyond the kernel of the same graph without the switch, in bytes, at V = 262 144
# (profiles/graph_events_mpe.md: the main lane's offset, its record, flags and held words of this vector and of the next one live next
# to a voice that already sits at the 128-register line)
EXTRA_SCRATCH_PITCH_GATE = 56
EXTRA_SCRATCH_MOD_Z = 120


def switched_forms(desc_outputs):
    """three_forms() of graphs built with the switch"""
    g = graph(desc_outputs, mpe_events=True)
    out = [("plain", *g.emit())]
    g.close()
    g = graph(desc_outputs, voice_list_events=True, mpe_events=True)
    out.append(("listed", *g.emit_listed()))
    g.close()
    g = graph(desc_outputs, group=16, voice_list_events=True, voice_list_groups=True, mpe_events=True)
    out.append(("lane plan", *g.emit_listed()))
    g.close()
    return out


PATCHES = [("pitch and gate", lambda: patches.synth16(pitch_input=True, event_rows=True)), ("z, mod and vox", rows_desc)]


@pytest.mark.parametrize("name,desc", PATCHES, ids=[p[0] for p in PATCHES])
def test_without_the_switch_no_source_names_the_new_structs(name, desc):
    for form, source, code in three_forms(desc()):
        assert "CtlVoiceMpe" not in source and "CtlRowsMpe" not in source, form
        assert "mlev::CtlVoice ev_0;" in source, form


@pytest.mark.parametrize("name,desc", PATCHES, ids=[p[0] for p in PATCHES])
def test_with_the_switch_the_plain_form_is_the_mpe_form_and_the_listed_forms_keep_their_text(name, desc):
    plain, listed, planned = three_forms(desc())
    s_plain, s_listed, s_planned = switched_forms(desc())
    source, code = s_plain[1], s_plain[2]
    assert code[:4] == b"\x7fELF" and "amdgcn-amd-amdhsa--gfx950" in _code_object_notes(code)
    assert "mlev::CtlVoiceMpe ev_0;" in source and "ev_0.load(a.events, v_0, a.T)" in source
    assert "mlev::CtlVoice ev_0;" not in source and "mlev::CtlRows<" not in source
    if name == "z, mod and vox":
        assert "mlev::CtlRowsMpe<76u> er_0;" in source and "er_0.load(a.events, v_0, a.T)" in source
    else:
        assert "CtlRows" not in source
    # apart from the structs' names the plain source is the one without the switch
    assert source.replace("CtlVoiceMpe", "CtlVoice").replace("CtlRowsMpe", "CtlRows") == plain[1]
    assert s_listed[1] == listed[1] and s_planned[1] == planned[1]


def test_the_switch_lifts_the_whole_wavefront_rule_of_a_mixed_down_output():
    """Event rows next to a mixed-down output ask for a multiple of 64 voices - not with the switch (nor with voice_list_events): the
    last wavefront's spare lanes run the last voice, its lane and its main lane, again."""
    desc, outputs = rows_desc()
    g = ml.Graph(ml.OfflineEngine(), 130, desc, outputs, compile_now=False)
    g.set_output_mixdown(0)
    refused(Status.ERR_UNSUPPORTED, ["whole wavefronts"], g.emit)
    g.close()
    g = ml.Graph(ml.OfflineEngine(), 130, desc, outputs, compile_now=False, mpe_events=True)
    g.set_output_mixdown(0)
    source, code = g.emit()
    assert "mlev::CtlVoiceMpe ev_0;" in source and "a.V - 1" in source and code[:4] == b"\x7fELF"
    g.close()


def test_register_budget_with_the_switch(monkeypatch):
    """The instrument bank's voice at 262 144 voices with the switch keeps the occupancy of the kernel without it - at most 128 VGPRs:
    four wavefronts per SIMD - and spills at most the pinned bytes more. From the code objects' notes."""
    monkeypatch.delenv("MLGPU_GRAPH_MIN_WAVES", raising=False)

    def budget(desc_outputs, **switches):
        g = graph(desc_outputs, V=262144, **switches)
        notes = _code_object_notes(g.emit()[1])
        g.close()
        return int(re.search(r"\.vgpr_count:\s+(\d+)", notes).group(1)), int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", notes).group(1))
    for name, desc, extra in (("pitch/gate only", patches.synth16(pitch_input=True, event_rows=True), EXTRA_SCRATCH_PITCH_GATE),
                              ("with mod and z", patches.synth16_mod_z(), EXTRA_SCRATCH_MOD_Z)):
        base_vgpr, base_scratch = budget(desc)
        vgpr, scratch = budget(desc, mpe_events=True)
        print(f"synth16 with event rows, V = 262144, {name}: without the switch {base_vgpr} VGPRs, {base_scratch} B private; with it {vgpr} VGPRs, {scratch} B private")
        assert base_vgpr <= 128 and vgpr <= 128, name
        assert scratch <= base_scratch + extra, name


def test_refusals_without_a_device():
    assert re.search(r"int\s+mlgpu_graph_enable_mpe_events\s*\(\s*mlgpu_graph\s*\*\s*g\s*,\s*int\s+on\s*\)\s*;", _header())
    desc, outputs = rows_desc()
    g = ml.Graph(ml.OfflineEngine(), 128, desc, outputs, compile_now=False)
    g.enable_mpe_events()
    g.enable_mpe_events(False)
    assert "CtlVoiceMpe" not in g.emit()[0]
    g.close()
    g = ml.Graph(ml.OfflineEngine(), 128, desc, outputs, compile_now=False, mpe_events=True)
    assert "CtlVoiceMpe" in g.emit()[0]
    g.close()


def test_the_python_keyword_matches_the_header():
    import inspect
    assert "mpe_events" in inspect.signature(ml.Graph.__init__).parameters
    assert inspect.signature(ml.Graph.__init__).parameters["mpe_events"].default is False
    assert "mlgpu_graph_enable_" + "mpe_events" in _header()
    assert hasattr(ml.Graph, "enable_mpe_events")
