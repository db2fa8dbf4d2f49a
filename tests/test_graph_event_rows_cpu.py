"""The event rows vox, z, x, y and mod as source nodes of a voice graph, without a device (mlgpu_graph_add_event_row, rows 2..6): the
three kernel forms of a graph that reads them hold mlev::CtlRows and compile for gfx950, a pitch/gate-only graph's sources do not name
it, the register budget of the instrument bank's voice with mod and z, the refusals. Engine-less graphs, as
tests/test_graph_voice_list_events_cpu.py makes them."""
import re

import pytest

import madronalib_amd as ml
from madronalib_amd import constants, patches
from madronalib_amd.constants import EventRow, Op, Status
from test_abi import _code_object_notes, _header
from test_graph_voice_list_cpu import refused

V = 2352
# What the voice with mod and z may keep in scratch beyond the pitch/gate-only kernel of the same bank, in bytes (the figure of
# profiles/graph_event_rows.md: two more row values per quad next to a voice that already sits at the 128-register line)
EXTRA_SCRATCH = 64


def rows_desc():
    """pitch, gate, mod, z and vox, all used: sine(pitch) * adsr(gate) * (1 + mod) + z * (vox + 1)."""
    d = [dict(name="pitch", type="event_row", kind=EventRow.PITCH), dict(name="gate", type="event_row", kind=EventRow.GATE),
         dict(name="mod", type="event_row", kind=EventRow.MOD), dict(name="z", type="event_row", kind=EventRow.Z),
         dict(name="vox", type="event_row", kind=EventRow.VOX), dict(name="one", type="const", value=1.0), dict(name="base", type="const", value=0.01),
         dict(name="ratio", type="op", kind=Op.EXP2_APPROX, inputs=["pitch"]), dict(name="freq", type="op", kind=Op.MULTIPLY, inputs=["ratio", "base"]),
         dict(name="osc", type="proc", kind=ml.Proc.SINE_GEN, inputs=["freq"]), dict(name="env", type="proc", kind=ml.Proc.ADSR, inputs=["gate"]),
         dict(name="amp", type="op", kind=Op.MULTIPLY, inputs=["osc", "env"]), dict(name="m1", type="op", kind=Op.ADD, inputs=["one", "mod"]),
         dict(name="wet", type="op", kind=Op.MULTIPLY, inputs=["amp", "m1"]), dict(name="v1", type="op", kind=Op.ADD, inputs=["vox", "one"]),
         dict(name="zv", type="op", kind=Op.MULTIPLY, inputs=["z", "v1"]), dict(name="out", type="op", kind=Op.ADD, inputs=["wet", "zv"])]
    return d, ["out"]


def graph(desc_outputs, V=V, group=0, **switches):
    desc, outputs = desc_outputs
    return ml.Graph(ml.OfflineEngine(), V, desc, outputs, output_groups={0: group} if group else None, compile_now=False, **switches)


def three_forms(desc_outputs):
    """(name, source, code object) of emit(), the plain listed form and the lane plan's with a group sum of 16."""
    g = graph(desc_outputs)
    out = [("plain", *g.emit())]
    g.close()
    g = graph(desc_outputs, voice_list_events=True)
    out.append(("listed", *g.emit_listed()))
    g.close()
    g = graph(desc_outputs, group=16, voice_list_events=True, voice_list_groups=True)
    out.append(("lane plan", *g.emit_listed()))
    g.close()
    return out


def test_python_enum_matches_the_header():
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(MLGPU_[A-Z0-9_]+)\s*=\s*(\d+)", _header())}
    names = [k for k, v in vars(constants.EventRow).items() if not k.startswith("_") and isinstance(v, int)]
    assert len(names) == 8
    for k in names:
        assert vals["MLGPU_EVENT_ROW_" + k] == getattr(constants.EventRow, k)
    assert [getattr(EventRow, n.upper()) for n in ml.Events.ROWS] == list(range(8))


def test_the_three_forms_of_a_graph_with_the_new_rows():
    """Each form is a gfx950 code object whose source holds mlev::CtlRows for the rows z, mod and vox (mask 0x4C), next to CtlVoice for
    pitch and gate; the listed forms load it by the gathered voice."""
    for name, source, code in three_forms(rows_desc()):
        assert code[:4] == b"\x7fELF" and "amdgcn-amd-amdhsa--gfx950" in _code_object_notes(code), name
        assert "mlev::CtlRows<76u> er_0;" in source and "mlev::CtlVoice ev_0;" in source, name
        assert "er_0.load(a.events, v_0, a.T)" in source, name
        for r in (EventRow.VOX, EventRow.Z, EventRow.MOD):
            assert f"er_0.row<{r}>(t, q)" in source, (name, r)
        assert "row<4>" not in source and "row<5>" not in source, name
        if name == "listed":
            assert "a.voiceList[" in source and "a.lanePlan" not in source
        if name == "lane plan":
            assert "a.lanePlan" in source and "segment_sum_store" in source


def test_rows_without_pitch_or_gate_make_no_ctlvoice():
    """A graph whose only event rows are among 2..6 is an events graph, and constructs CtlVoice only if it needs it."""
    desc = [dict(name="x", type="event_row", kind=EventRow.X), dict(name="y", type="event_row", kind=EventRow.Y),
            dict(name="xy", type="op", kind=Op.MULTIPLY, inputs=["x", "y"])]
    g = graph((desc, ["xy"]), V=128)
    source, code = g.emit()
    assert "mlev::CtlRows<48u> er_0;" in source and "mlev::CtlVoice" not in source and code[:4] == b"\x7fELF"
    g.close()


def test_pitch_and_gate_only_sources_do_not_name_the_new_struct():
    for name, source, code in three_forms(patches.synth16(pitch_input=True, event_rows=True)):
        assert "CtlRows" not in source and "mlev::CtlVoice ev_0;" in source, name


def test_register_budget_with_mod_and_z(monkeypatch):
    """The instrument bank's voice reading mod and z (patches.synth16_mod_z) at 262 144 voices keeps the occupancy of the
    pitch/gate-only kernel - at most 128 VGPRs: four wavefronts per SIMD - and spills at most EXTRA_SCRATCH bytes more. From the
    code objects' notes."""
    monkeypatch.delenv("MLGPU_GRAPH_MIN_WAVES", raising=False)

    def budget(desc_outputs):
        g = graph(desc_outputs, V=262144)
        notes = _code_object_notes(g.emit()[1])
        g.close()
        return int(re.search(r"\.vgpr_count:\s+(\d+)", notes).group(1)), int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", notes).group(1))
    base_vgpr, base_scratch = budget(patches.synth16(pitch_input=True, event_rows=True))
    vgpr, scratch = budget(patches.synth16_mod_z())
    print(f"synth16 with event rows, V = 262144: pitch/gate only {base_vgpr} VGPRs, {base_scratch} B private; with mod and z {vgpr} VGPRs, {scratch} B private")
    assert base_vgpr <= 128 and vgpr <= 128
    assert scratch <= base_scratch + EXTRA_SCRATCH


def test_refusals():
    g = ml.Graph(ml.OfflineEngine(), 64, compile_now=False)
    for row in (EventRow.TIME, -1, 8):
        refused(Status.ERR_UNSUPPORTED, [], g.add, f"r{row}", "event_row", row)
    g.add("mod", "event_row", EventRow.MOD)
    refused(Status.ERR_INVALID, [], g.add, "mod2", "event_row", EventRow.MOD)
    for row in (EventRow.PITCH, EventRow.GATE, EventRow.VOX, EventRow.Z, EventRow.X, EventRow.Y):
        g.add(f"row{row}", "event_row", row)
    g.close()
