"""Voice records (mlgpu_graph_export_voices / _import_voices and the bank's) where no GPU is needed: the host planner under the
sanitizers, the new symbols through the layers, and what an object without a device answers."""
import os
import re
import subprocess

import pytest

import madronalib_amd as ml
from madronalib_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madronalib_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "mlgpu.h")
SYMBOLS = [f"mlgpu_{owner}_{name}" for owner in ("graph", "bank")
           for name in ("voice_record_words", "voice_record_signature", "reserve_voice_records", "export_voices", "import_voices")]


def test_record_planner_under_sanitizers(tmp_path):
    """tests/cpp/voice_records_plan_test.cpp: a host model of the tables and of ring memory in which every word holds its own address;
    the planned gather and scatter, applied with plain loops, against a brute-force walk of the address map - granules 1, 8 and 16,
    voices at the 256-block borders, two ring nodes one of them with two rings, a bank without rings, the spare lanes of layout 2 -
    then the signature's equalities and inequalities and the host-side refusals. Built with g++ -fsanitize=address,undefined from the
    planner's one file and run directly."""
    if not os.path.exists("/usr/bin/g++"):
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    pb = subprocess.run(["g++", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=300)
    if pb.returncode != 0:
        pytest.skip("sanitizer runtime not installed: " + pb.stderr[-200:])
    exe = str(tmp_path / "voice_records_plan_test")
    planner = os.path.join(CSRC, "voice_records.cpp")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cpp", "voice_records_plan_test.cpp"), planner, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    used = subprocess.run(["g++", "-std=c++17", "-M", planner], capture_output=True, text=True, timeout=300).stdout
    assert "hip/" not in used and "hip_runtime" not in used and "voice_records.hpp" in used and "param_updates.hpp" in used
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_symbols_through_the_layers():
    """The header declares the ten calls, the library exports them, and both Python classes have the five names."""
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
    assert re.search(r"int\s+mlgpu_graph_import_voices\(mlgpu_graph\*\s*g,\s*uint64_t\s+signature,\s*const uint32_t\*\s*h_voices,\s*size_t\s+n,\s*const uint32_t\*\s*d_records\)", header)
    for cls in (ml.Graph, ml.Bank):
        for name in ("voice_record_words", "voice_record_signature", "reserve_voice_records", "export_voices", "import_voices"):
            assert hasattr(cls, name), (cls, name)


def test_graph_that_is_not_compiled():
    """A graph without an engine is never compiled: no record words, no signature, and every call says so."""
    from madronalib_amd.constants import Proc
    g = ml.Graph(ml.OfflineEngine(), 256)
    g.add("x", "input")
    g.add("d", "proc", Proc.INTEGER_DELAY, ["x"], max_delay=100.0)
    g.add_output("d")
    g.emit()
    assert g.voice_record_words == 0 and g.voice_record_signature == 0
    for call in (lambda: g.reserve_voice_records(16), lambda: g.export_voices([1, 2], 4096), lambda: g.import_voices(0, [1, 2], 4096)):
        with pytest.raises(ml.MlgpuError) as ei:
            call()
        assert ei.value.status == ml.Status.ERR_INVALID and "compile first" in str(ei.value)
    assert g.L.mlgpu_graph_export_voices(None, None, 0, None) == ml.Status.ERR_INVALID
    assert g.L.mlgpu_bank_import_voices(None, 0, None, 0, None) == ml.Status.ERR_INVALID
    assert g.L.mlgpu_bank_voice_record_words(None) == 0 and g.L.mlgpu_graph_voice_record_signature(None) == 0
    g.close()


def test_documents_name_the_calls():
    for doc, words in (("INTEGRATION.md", ["Moving voices", "mlgpu_graph_export_voices", "mlgpu_graph_import_voices", "VoiceBank"]),
                       ("README.md", ["mlgpu_graph_export_voices"]), ("DESIGN.md", ["voice_records.hip"]), (os.path.join("profiles", "voice_records.md"), ["export", "import"])):
        text = open(os.path.join(ROOT, doc)).read()
        for w in words:
            assert w in text, (doc, w)
