"""Voice lists for graphs, without a device: the listed form of a graph's generated kernel (mlgpu_graph_emit_listed), the plain kernel's
source left byte for byte as it is, the refusals planGraph decides, and the calls on a graph made without
mlgpu_graph_enable_voice_lists. Engine-less graphs throughout, as tests/test_abi.py makes them."""
import types

import pytest

import madronalib_amd as ml
from graph_voice_list_cases import build_graph, string_desc, synth_desc, three_ring_desc, upsample_graph
from madronalib_amd.constants import Region, Status
from test_abi import _code_object_notes

V = 2352


def case_of(desc_outputs, mix=()):
    desc, outputs = desc_outputs
    return types.SimpleNamespace(desc=desc, outputs=outputs, mix=mix, inputs={n["name"]: None for n in desc if n["type"] == "input"}, groups={})


def offline(desc_outputs, mix=(), voice_lists=True, delay_windows=False, V=V):
    return build_graph(ml.OfflineEngine(), case_of(desc_outputs, mix), V, voice_lists, delay_windows)


def refused(status, words, fn, *args):
    with pytest.raises(ml.MlgpuError) as ei:
        fn(*args)
    assert ei.value.status == status, str(ei.value)
    assert all(w in str(ei.value) for w in words), str(ei.value)


def test_emit_listed_gives_a_gfx950_code_object():
    """The synth voice - an oscillator trip pair, an input, a Lopass, a control, a plain and a mixed-down output: its listed kernel
    reads its voice from the list, keeps the spare lanes of a last wavefront for the mixdown tree, and compiles for gfx950."""
    g = offline(synth_desc(), mix=(1,))
    source, code = g.emit_listed()
    assert "mlgpu_graph_listed_kernel" in source and "a.voiceList[" in source and "a.listed" in source and "a.peaks" in source
    assert "trip_locked" in source and "mix64_park" in source
    assert code[:4] == b"\x7fELF"
    notes = _code_object_notes(code)
    assert "amdgcn-amd-amdhsa--gfx950" in notes and "mlgpu_graph_listed_kernel" in notes
    assert g.listed_source() == source
    plain_source, plain_code = g.emit()
    assert plain_code[:4] == b"\x7fELF" and plain_source != source
    g.close()


@pytest.mark.parametrize("which", ["synth", "string"])
def test_the_plain_source_is_unchanged(which):
    """With voice lists enabled the kernel of mlgpu_graph_process is generated from the same text as without."""
    desc, mix = (synth_desc(), (1,)) if which == "synth" else (string_desc(), ())
    on, off = offline(desc, mix, True), offline(desc, mix, False)
    on.emit(), off.emit()
    assert on.source == off.source and len(on.source) > 1000
    assert "voiceList" not in on.source and "a.listed" not in on.source and "a.peaks" not in on.source
    assert on.listed_source() and off.listed_source() == ""
    refused(Status.ERR_INVALID, ["graph_emit_listed", "mlgpu_graph_enable_voice_lists"], off.emit_listed)
    on.close(), off.close()


def _group_sum(voice_lists):
    g = offline(synth_desc(), voice_lists=voice_lists, V=2352)
    g.set_output_group_sum(0, 16)
    return g


def _shard(voice_lists):
    g = build_graph(ml.OfflineEngine(), case_of(synth_desc()), 2304, voice_lists)     # (the shard form wants whole 64-voice groups)
    g.set_output_mixdown(1, "shard")
    return g


def _event_rows(voice_lists):
    desc = [dict(name="gate", type="event_row", kind=1), dict(name="env", type="proc", kind=ml.Proc.ADSR, inputs=["gate"])]
    return offline((desc, ["env"]), voice_lists=voice_lists)


REFUSALS = {
    "layout1": (lambda vl: offline(string_desc(), voice_lists=vl, delay_windows=1), ["delay layout 1", "mlgpu_graph_set_delay_layout(g, 0)"]),
    "layout2": (lambda vl: offline(string_desc(), voice_lists=vl, delay_windows=2), ["delay layout 2", "mlgpu_graph_set_delay_layout(g, 0)"]),
    "layout4": (lambda vl: offline(string_desc(), voice_lists=vl, delay_windows=4), ["delay layout 4", "mlgpu_graph_set_delay_layout(g, 0)"]),
    "layout3_one_ring": (lambda vl: offline(string_desc(), voice_lists=vl, delay_windows=3), ["delay layout 2", "layout 3 resolves", "mlgpu_graph_set_delay_layout(g, 0)"]),
    "layout3_three_rings": (lambda vl: offline(three_ring_desc(), voice_lists=vl, delay_windows=3), ["delay layout 4", "layout 3 resolves"]),
    "group_sum": (_group_sum, ["group sum"]),
    "mixdown_shard": (_shard, ["shard"]),
    "event_rows": (_event_rows, ["event rows"]),
    "downsample": (lambda vl: upsample_graph(ml.OfflineEngine(), V, vl, Region.DOWNSAMPLE_2X), ["DOWNSAMPLE_2X"]),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_graphs_the_listed_form_does_not_serve_are_refused_at_emit(name):
    """MLGPU_ERR_UNSUPPORTED from both emits, the message names the reason and nothing is built; the same graph without voice lists
    still emits."""
    make, words = REFUSALS[name]
    g = make(True)
    for emit in (g.emit_listed, g.emit):
        refused(Status.ERR_UNSUPPORTED, ["voice lists"] + words, emit)
        assert g.source == "" and g.listed_source() == ""
    g.close()
    g = make(False)
    source, code = g.emit()
    assert code[:4] == b"\x7fELF"
    g.close()


@pytest.mark.parametrize("rings", [1, 3])
def test_ring_layout_0_is_served(rings):
    """The rows: one ring, and three - where the plan issues the ring reads early, by LDS-DMA into landing slots per lane."""
    g = offline(string_desc() if rings == 1 else three_ring_desc())
    source, code = g.emit_listed()
    assert code[:4] == b"\x7fELF" and "a.voiceList[" in source
    assert ("ldsEarly" in source) == (rings == 3)
    assert g.delay_layout == 0
    g.close()


def test_the_served_kinds_emit():
    """An UPSAMPLE_2X region and an input group."""
    g = upsample_graph(ml.OfflineEngine(), V)
    assert g.emit_listed()[1][:4] == b"\x7fELF"
    g.close()
    case = case_of(synth_desc(), (1,))
    case.groups = {"x": 16}
    g = build_graph(ml.OfflineEngine(), case, V)
    source, code = g.emit_listed()
    assert code[:4] == b"\x7fELF" and "(v_0 / 16)" in source
    g.close()


def test_a_graph_made_without_voice_lists_says_so():
    g = offline(synth_desc(), (1,), voice_lists=False)
    g.emit()
    refused(Status.ERR_INVALID, ["graph_set_voice_list", "mlgpu_graph_enable_voice_lists", "before compile"], g.set_voice_list, [1, 2, 3])
    refused(Status.ERR_INVALID, ["graph_reserve_voice_list", "mlgpu_graph_enable_voice_lists", "before compile"], g.reserve_voice_list, 8)
    refused(Status.ERR_INVALID, ["graph_process_listed", "mlgpu_graph_enable_voice_lists", "before compile"], g.process_listed, 1, [0], [0, 0], 0, 0, [0])
    assert g.voice_list_size == 0
    g.close()


def test_an_ahead_of_time_async_compile_makes_both_kernels():
    """mlgpu_graph_compile_async on an engine-less graph with voice lists: when the poll says ready, both sources are there and both
    code objects come out of the caches."""
    import time
    g = build_graph(ml.OfflineEngine(), case_of(synth_desc(), (1,)), 4608, True)     # (a size no other test compiles)
    g.compile_async()
    while not g.compile_poll():
        time.sleep(0.001)
    assert "mlgpu_graph_kernel" in g.source and "mlgpu_graph_listed_kernel" in g.listed_source()
    assert g.emit()[1][:4] == b"\x7fELF" and g.emit_listed()[1][:4] == b"\x7fELF"
    g.close()
