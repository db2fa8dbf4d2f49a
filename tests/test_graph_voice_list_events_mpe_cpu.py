"""The build switch mlgpu_graph_enable_voice_list_mpe_events without a device: with it off every form's source is what it is without
mpe_events; with it on the listed and the lane-plan sources are the unswitched ones but for the names of mlev::CtlVoiceMpe /
mlev::CtlRowsMpe, loaded with the gathered voice, and compile for gfx950; what the switch turns on and what turns it off; the header
and the Python interface; the compiler's register and scratch figures of the instrument bank's listed kernels with and without the
switch. Engine-less graphs, as tests/test_graph_event_rows_cpu.py makes them."""
import inspect
import re

import pytest

import madronalib_amd as ml
from madronalib_amd import patches
from madronalib_amd.constants import Status
from test_abi import _code_object_notes, _header
from test_graph_event_rows_cpu import graph, rows_desc, three_forms
from test_graph_voice_list_cpu import refused

PATCHES = [("pitch and gate", lambda: patches.synth16(pitch_input=True, event_rows=True)), ("z, mod and vox", rows_desc)]


def forms(desc_outputs, **switches):
    """three_forms() of graphs built with `switches` beside those each form needs"""
    g = graph(desc_outputs, **switches)
    out = [("plain", *g.emit())]
    g.close()
    g = graph(desc_outputs, voice_list_events=True, **switches)
    out.append(("listed", *g.emit_listed()))
    g.close()
    g = graph(desc_outputs, group=16, voice_list_events=True, voice_list_groups=True, **switches)
    out.append(("lane plan", *g.emit_listed()))
    g.close()
    return out


def unswitched(source):
    return source.replace("CtlVoiceMpe", "CtlVoice").replace("CtlRowsMpe", "CtlRows")


@pytest.mark.parametrize("name,desc", PATCHES, ids=[p[0] for p in PATCHES])
def test_switch_off_every_source_is_the_one_without_mpe_events(name, desc):
    """mpe_events + voice_list_events (+ groups) without the new switch: the listed and lane-plan sources are those of graphs built
    without mpe_events, byte for byte, and the plain one differs by the struct names alone - as before the switch existed."""
    plain, listed, planned = three_forms(desc())
    m_plain, m_listed, m_planned = forms(desc(), mpe_events=True)
    assert m_listed[1] == listed[1] and m_planned[1] == planned[1]
    assert "CtlVoiceMpe" not in m_listed[1] and "CtlRowsMpe" not in m_listed[1] and "CtlVoiceMpe" not in m_planned[1] and "CtlRowsMpe" not in m_planned[1]
    assert unswitched(m_plain[1]) == plain[1] and "mlev::CtlVoiceMpe ev_0;" in m_plain[1]
    # ... and so when the switch was turned on and off again
    desc_, outputs = desc()
    for group in (0, 16):
        g = ml.Graph(ml.OfflineEngine(), 2352, desc_, outputs, output_groups={0: group} if group else None, compile_now=False,
                     voice_list_groups=bool(group))
        g.enable_voice_list_mpe_events()
        g.enable_voice_list_mpe_events(False)      # (what it turned on stays on: voice_list_events and mpe_events)
        assert g.emit_listed()[0] == (planned if group else listed)[1]
        assert "mlev::CtlVoiceMpe ev_0;" in g.emit()[0]
        g.close()


@pytest.mark.parametrize("name,desc", PATCHES, ids=[p[0] for p in PATCHES])
def test_switch_on_the_listed_forms_are_the_mpe_forms(name, desc):
    plain, listed, planned = three_forms(desc())
    m_plain = forms(desc(), mpe_events=True)[0]
    for base, (form, source, code) in zip((plain, listed, planned), forms(desc(), voice_list_mpe_events=True)):
        assert code[:4] == b"\x7fELF" and "amdgcn-amd-amdhsa--gfx950" in _code_object_notes(code), form
        assert "mlev::CtlVoiceMpe ev_0;" in source and "ev_0.load(a.events, v_0, a.T)" in source, form
        assert "mlev::CtlVoice ev_0;" not in source and "mlev::CtlRows<" not in source, form
        if name == "z, mod and vox":
            assert "mlev::CtlRowsMpe<76u> er_0;" in source and "er_0.load(a.events, v_0, a.T)" in source, form
        else:
            assert "CtlRows" not in source, form
        # loaded with the gathered voice: v_0 is the list's or the lane plan's entry
        if form == "listed":
            assert "a.voiceList[" in source and "a.lanePlan" not in source
        if form == "lane plan":
            assert "a.lanePlan" in source and "segment_sum_store" in source
        # apart from the structs' names the source is the one without the switch
        assert unswitched(source) == base[1], form
        if form == "plain":
            assert source == m_plain[1]      # (the switch turns mpe_events on)


def test_what_the_switch_turns_on_and_what_turns_it_off():
    desc, outputs = rows_desc()

    def listed_source(*calls, **kw):
        g = ml.Graph(ml.OfflineEngine(), 128, desc, outputs, compile_now=False, **kw)
        for c, on in calls:
            getattr(g, c)(on)
        try:
            return g.emit_listed()[0], g.emit()[0]
        finally:
            g.close()
    # on alone: voice lists, their events form and mpe_events come with it
    listed, plain = listed_source(("enable_voice_list_mpe_events", True))
    assert "mlev::CtlVoiceMpe ev_0;" in listed and "mlev::CtlVoiceMpe ev_0;" in plain
    # mpe_events off: the switch goes with it, voice_list_events stays
    listed, plain = listed_source(("enable_voice_list_mpe_events", True), ("enable_mpe_events", False))
    assert "CtlVoiceMpe" not in listed and "mlev::CtlVoice ev_0;" in listed and "CtlVoiceMpe" not in plain
    listed, plain = listed_source(("enable_mpe_events", False), ("enable_mpe_events", True), voice_list_mpe_events=True)
    assert "CtlVoiceMpe" not in listed and "mlev::CtlVoiceMpe ev_0;" in plain
    # voice lists off: the switch goes with the rest - no listed form at all, and turning voice lists on again does not bring it back
    g = ml.Graph(ml.OfflineEngine(), 128, desc, outputs, compile_now=False, voice_list_mpe_events=True)
    g.enable_voice_lists(False)
    refused(Status.ERR_INVALID, ["no listed form"], g.emit_listed)
    g.enable_voice_list_events()
    assert "CtlVoiceMpe" not in g.emit_listed()[0] and "mlev::CtlVoiceMpe ev_0;" in g.emit()[0]
    g.close()
    # the keyword next to the others
    g = ml.Graph(ml.OfflineEngine(), 128, desc, outputs, compile_now=False, voice_lists=True, voice_list_events=True, mpe_events=True, voice_list_mpe_events=True)
    assert "mlev::CtlVoiceMpe ev_0;" in g.emit_listed()[0]
    g.close()


def test_a_mixed_down_listed_form_at_130_voices_emits():
    """V = 130, the output mixed down: the listed form's last wavefront keeps its spare lanes - they run the list's last voice, its lane
    and its main lane, again - and compiles."""
    desc, outputs = rows_desc()
    g = ml.Graph(ml.OfflineEngine(), 130, desc, outputs, compile_now=False, voice_list_mpe_events=True)
    g.set_output_mixdown(0)
    source, code = g.emit_listed()
    assert "mlev::CtlVoiceMpe ev_0;" in source and "mlev::CtlRowsMpe<76u> er_0;" in source and "a.listed - 1" in source
    assert code[:4] == b"\x7fELF" and "amdgcn-amd-amdhsa--gfx950" in _code_object_notes(code)
    plain, pcode = g.emit()
    assert "mlev::CtlVoiceMpe ev_0;" in plain and "a.V - 1" in plain and pcode[:4] == b"\x7fELF"
    g.close()


def test_header_and_python():
    h = _header()
    assert re.search(r"int\s+mlgpu_graph_enable_voice_list_mpe_events\s*\(\s*mlgpu_graph\s*\*\s*g\s*,\s*int\s+on\s*\)\s*;", h)
    assert re.search(r"int\s+mlgpu_events_sounding_graph_voices\s*\(\s*mlgpu_events\s*\*\s*ev\s*,\s*uint32_t\s*\*\s*h_voices\s*,\s*size_t\s+capacity\s*,\s*size_t\s*\*\s*n\s*\)\s*;", h)
    p = inspect.signature(ml.Graph.__init__).parameters
    assert "voice_list_mpe_events" in p and p["voice_list_mpe_events"].default is False
    assert inspect.signature(ml.Graph.enable_voice_list_mpe_events).parameters["on"].default is True
    assert hasattr(ml.Events, "sounding_graph_voices") and hasattr(ml.Events, "sounding_voices")
    # the header no longer states the MIDI-only limit of the listed forms without naming the switch
    at = h.index("The listed forms are not served")
    assert "mlgpu_graph_enable_voice_list_mpe_events" in h[at:at + 600] and "mlgpu_events_sounding_graph_voices" in h[at:at + 600]


# The compiler's figures at V = 262 144, read from the code objects on the build machine (profiles/graph_voice_list_events_mpe.md):
# (VGPRs, private-segment bytes) of the two listed forms, without the switch (voice_list_events alone) and with it. Upper bounds.
# Wavefronts per SIMD, floor(512 / VGPRs): synth16 list form 3 -> 3, lane plan 3 -> 2; synth16_mod_z list form 3 -> 2, lane plan 3 -> 2.
FIGURES = {
    ("synth16", "listed"): ((129, 0), (144, 0)),
    ("synth16", "lane plan"): ((157, 0), (173, 0)),
    ("synth16_mod_z", "listed"): ((145, 0), (176, 0)),
    ("synth16_mod_z", "lane plan"): ((168, 0), (204, 0)),
}


def test_register_and_scratch_figures_of_the_listed_forms(monkeypatch):
    monkeypatch.delenv("MLGPU_GRAPH_MIN_WAVES", raising=False)

    def figures(desc_outputs, group, **switches):
        g = graph(desc_outputs, V=262144, group=group, voice_list_groups=bool(group), **switches)
        notes = _code_object_notes(g.emit_listed()[1])
        g.close()
        return int(re.search(r"\.vgpr_count:\s+(\d+)", notes).group(1)), int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", notes).group(1))
    for patch, desc in (("synth16", lambda: patches.synth16(pitch_input=True, event_rows=True)), ("synth16_mod_z", patches.synth16_mod_z)):
        for form, group in (("listed", 0), ("lane plan", 16)):
            base = figures(desc(), group, voice_list_events=True)
            with_switch = figures(desc(), group, voice_list_mpe_events=True)
            print(f"{patch}, V = 262144, {form}: without the switch {base[0]} VGPRs ({512 // base[0]} wavefronts per SIMD), {base[1]} B private; "
                  f"with it {with_switch[0]} VGPRs ({512 // with_switch[0]} wavefronts per SIMD), {with_switch[1]} B private")
            pinned_base, pinned_switch = FIGURES[patch, form]
            assert base[0] <= pinned_base[0] and base[1] <= pinned_base[1], (patch, form, base)
            assert with_switch[0] <= pinned_switch[0] and with_switch[1] <= pinned_switch[1], (patch, form, with_switch)
