"""Sparse, stream-ordered updates of per-voice params, coefficients and state (mlgpu_graph_apply_updates / mlgpu_bank_apply_updates).

Bits, not tolerances, and the yardstick is the whole-row API: a twin object is changed with set_param / set_coeff / set_state /
set_input_const arrays made by the naive model "apply the records one at a time, in list order", the object under test gets the
records; tables (get_param, get_coeff, get_state of every word) and outputs must be the same words. Shapes: 80 voices (a quarter of
a wavefront past the first, dead lanes) and 2 352 (nine workgroups and a partial last wavefront), the sizes the bank tests use."""
import os
import subprocess

import numpy as np
import pytest

import madronalib_amd as ml
from inputs import gate_signal, lcg_noise
from madronalib_amd.constants import Op, Proc, Status

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENORMAL, NEG_ZERO, NAN_BITS = 0x00000001, 0x80000000, 0x7FC00123
SIZES = [80, 2352]


@pytest.fixture(scope="module")
def eng():
    e = ml.Engine(0)
    yield e
    e.close()


def staging(obj):
    """(the four staging buffer addresses, the capacity in records) of a graph's or bank's update staging sets: the library's test hook."""
    import ctypes
    fn = getattr(obj.L, "mlgpu_graph_update_staging" if isinstance(obj, ml.Graph) else "mlgpu_bank_update_staging")
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    four = (ctypes.c_void_p * 4)()
    cap = fn(obj.h, four)
    return tuple(four), int(cap)


def same(a, b):
    return bool((np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all())


def fbits(x):
    return int(np.float32(x).view(np.uint32))


# ---- the voice graph: param -> LinearGlide -> SawGen -> Lopass, gated by an ADSR on the streamed input (or by the input itself),
# ---- with a one-vector feedback around it
def voice_desc(adsr=True):
    d = [dict(name="gate", type="input"), dict(name="pitch", type="param"), dict(name="half", type="const", value=0.5),
         dict(name="glide", type="proc", kind=Proc.LINEAR_GLIDE, inputs=["pitch"]),
         dict(name="saw", type="proc", kind=Proc.SAW_GEN, inputs=["glide"]),
         dict(name="lp", type="proc", kind=Proc.LOPASS, inputs=["saw"])]
    if adsr:
        d += [dict(name="env", type="proc", kind=Proc.ADSR, inputs=["gate"]), dict(name="out", type="op", kind=Op.MULTIPLY, inputs=["lp", "env"])]
    else:
        d += [dict(name="out", type="op", kind=Op.MULTIPLY, inputs=["lp", "gate"])]
    d += [dict(name="fb", type="feedback", source="mix"), dict(name="fbs", type="op", kind=Op.MULTIPLY, inputs=["fb", "half"]),
          dict(name="mix", type="op", kind=Op.ADD, inputs=["out", "fbs"])]
    return d


def make_voice(eng, V, adsr=True):
    g = ml.Graph(eng, V, voice_desc(adsr), ["mix"])
    g.clear()
    g.set_param("pitch", (0.002 + 0.01 * ((np.arange(V) * 7) % 31) / 31.0).astype(np.float32))
    g.set_coeffs("glide", [float(c) for c in ml.LinearGlide.makeCoeffs(192.0)])
    g.set_coeffs("lp", [float(c) for c in ml.Lopass.makeCoeffs(0.12, 0.8)])
    if adsr:
        g.set_coeffs("env", [float(c) for c in ml.ADSR.calcCoeffs(0.002, 0.004, 0.6, 0.003, 48000.0)])
    return g


def rows_of(g):
    """Every table row of a graph as (kind, node name, index): 'p' params, 'c' coefficients, 's' state."""
    keys = []
    for name, nid in g.ids.items():
        nc, ns = g.L.mlgpu_graph_num_coeffs(g.h, nid), g.L.mlgpu_graph_num_state(g.h, nid)
        if name == "pitch":
            keys.append(("p", name, 0))
        keys += [("c", name, i) for i in range(max(nc, 0))] + [("s", name, i) for i in range(max(ns, 0))]
    return keys


def read_tables(g, keys=None):
    out = {}
    for k in (keys if keys is not None else rows_of(g)):
        kind, name, i = k
        a = g.get_param(name) if kind == "p" else (g.get_coeff(name, i) if kind == "c" else g.get_state(name, i))
        out[k] = a.view(np.uint32).copy()
    return out


def model_apply(tables, ops):
    """The naive model: each op (kind, name, index, first, n, bits) in list order; returns the rows touched."""
    touched = []
    for kind, name, i, first, n, bits in ops:
        tables[(kind, name, i)][first:first + n] = bits
        if (kind, name, i) not in touched:
            touched.append((kind, name, i))
    return touched


def set_whole_rows(g, tables, keys):
    for kind, name, i in keys:
        row = tables[(kind, name, i)]
        if kind == "p":
            g.set_param(name, row.view(np.float32))
        elif kind == "c":
            g.set_coeff(name, i, row.view(np.float32))
        else:
            g.set_state(name, i, row)


def records(g, ops):
    make = {"p": lambda nid, i, f, n, b: ml.Update(nid, 0, 0, f, n, b), "c": lambda nid, i, f, n, b: ml.Update(nid, 1, i, f, n, b),
            "s": lambda nid, i, f, n, b: ml.Update(nid, 2, i, f, n, b)}
    return [make[kind](g.ids[name], i, first, n, bits) for kind, name, i, first, n, bits in ops]


def assert_tables_equal(a, b, what, keys=None):
    for k in (keys if keys is not None else a):
        assert same(a[k], b[k]), (what, k, np.flatnonzero(a[k] != b[k])[:8])


def coverage_ranges(V):
    """n = 1, the last voice, [60, 70) across a wavefront, [250, 270) across a workgroup (where the bank has one), the whole bank."""
    r = [(0, V), (3, 1), (V - 1, 1), (60, 10)]
    return r + ([(250, 20)] if V >= 270 else [])


def lopass_ops(first, n, omega, k):
    """The three coefficients of one Lopass design for a range (coefficients of different designs mixed in one voice need not be a
    stable filter, and a bank of NaNs compares nothing)."""
    return [("c", "lp", i, first, n, fbits(c)) for i, c in enumerate(ml.Lopass.makeCoeffs(omega, k))]


def coverage_ops(V):
    """Every range with every target; the denormal, the -0.0 and the NaN pattern ride on the short ranges, after the whole-bank
    records they lie over."""
    ops = []
    for first, n in coverage_ranges(V):
        whole = n == V
        ops.append(("p", "pitch", 0, first, n, fbits(0.004) if whole else (DENORMAL if n == 1 and first == 3 else fbits(0.006 + 0.0001 * first))))
        ops += lopass_ops(first, n, 0.1 if whole else 0.05 + 0.0005 * first, 0.75)
        if first == V - 1:
            ops.append(("c", "lp", 1, first, n, NEG_ZERO))
        ops.append(("s", "lp", 0, first, n, fbits(0.01) if whole else (NAN_BITS if first == 60 else (DENORMAL if first == 3 else fbits(-0.02)))))
        ops.append(("s", "fb", 63, first, n, NEG_ZERO if first == V - 1 else fbits(0.003)))
    return ops


def random_ops(V, n, seed, max_len=20):
    rng = np.random.default_rng(seed)
    ops = []
    while len(ops) < n:
        first = int(rng.integers(0, V))
        cnt = int(min(V - first, rng.integers(1, max_len + 1)))
        t = int(rng.integers(0, 5))
        if t == 0 or (t in (1, 4) and n - len(ops) < 3):
            ops.append(("p", "pitch", 0, first, cnt, fbits(rng.uniform(0.001, 0.02))))
        elif t == 1:
            ops += lopass_ops(first, cnt, float(rng.uniform(0.02, 0.3)), float(rng.uniform(0.4, 1.2)))
        elif t == 2:
            ops.append(("s", "lp", int(rng.integers(0, 2)), first, cnt, fbits(rng.uniform(-0.5, 0.5))))
        elif t == 3:
            ops.append(("s", "fb", int(rng.integers(0, 64)), first, cnt, fbits(rng.uniform(-0.1, 0.1))))
        else:
            ops += [("c", "glide", i, first, cnt, fbits(c)) for i, c in enumerate(ml.LinearGlide.makeCoeffs(64.0 * float(rng.integers(1, 9))))]
    return ops


@pytest.mark.gpu
@pytest.mark.parametrize("flush", [False, True])
@pytest.mark.parametrize("V", SIZES)
def test_twin_graphs(eng, V, flush):
    """One twin changed with whole-row arrays, the other with the equivalent records - lists of 1, 64, 65 and 1 000 records and the
    ranges of coverage_ranges - over three launches: outputs, every state word, params and coefficients equal after each; what was
    written (a denormal, a -0.0 and a NaN pattern among it) is in the tables as given, also when the engine flushes denormals."""
    T = 2
    eng.set_flush_denormals(flush)
    try:
        a, b = make_voice(eng, V), make_voice(eng, V)
        keys = rows_of(b)
        assert len([k for k in keys if k[0] == "s"]) >= 64 + 60 and ("p", "pitch", 0) in keys and ("c", "lp", 2) in keys
        lists = [[coverage_ops(V), random_ops(V, 1, 1)], [random_ops(V, 64, 2), random_ops(V, 65, 3)], [random_ops(V, 1000, 4)]]
        for launch, calls in enumerate(lists):
            model = read_tables(a, keys)
            for ops in calls:
                touched = model_apply(model, ops)
                set_whole_rows(a, model, touched)
                recs = records(b, ops)
                assert b.update_device_records(recs) == len(recs)
                b.apply_updates(recs)
                assert_tables_equal(read_tables(b, touched), model, f"as given, launch {launch}", touched)
            sig = {"gate": gate_signal(V, 64 * T, 10 + launch)}
            (ya,), (yb,) = a.process_host(T, sig), b.process_host(T, sig)
            assert same(ya, yb), (launch, np.flatnonzero((ya.view(np.uint32) != yb.view(np.uint32)).any(1))[:8])
            assert_tables_equal(read_tables(a, keys), read_tables(b, keys), f"after launch {launch}")
        ok = np.isfinite(ya).all(1)
        assert ok.sum() > V // 2 and np.abs(ya[ok]).max() > 1e-4
        a.close()
        b.close()
    finally:
        eng.set_flush_denormals(False)


@pytest.mark.gpu
def test_later_record_wins(eng):
    """Two records on one word in one call: the later one is there. Then 600 random records on a few rows of 80 voices, ranges up to
    40 voices long - nearly every record lies over an earlier one - against the naive model."""
    V = 80
    g = make_voice(eng, V)
    g.apply_updates([ml.Update.param(g.ids["pitch"], 10, 20, 0.25), ml.Update.param(g.ids["pitch"], 15, 1, 0.5),
                     ml.Update.param(g.ids["pitch"], 29, 5, 0.75), ml.Update.param(g.ids["pitch"], 15, 1, 0.125)])
    want = g.get_param("pitch")
    assert want[15] == 0.125 and want[14] == 0.25 and want[16] == 0.25 and want[28] == 0.25 and want[29] == 0.75 and want[33] == 0.75
    keys = rows_of(g)
    model = read_tables(g, keys)
    rng = np.random.default_rng(7)
    rows = [("p", "pitch", 0), ("c", "lp", 0), ("s", "lp", 1), ("s", "fb", 5)]
    ops = []
    for j in range(600):
        first = int(rng.integers(0, V))
        ops.append(rows[int(rng.integers(0, len(rows)))] + (first, int(min(V - first, rng.integers(1, 41))), 0x3C000000 + j))
    model_apply(model, ops)
    g.apply_updates(records(g, ops))
    assert_tables_equal(read_tables(g, keys), model, "600 overlapping records")
    assert staging(g)[1] >= 1024                         # no reserve: both sets grew inside the two calls
    g.close()


@pytest.mark.gpu
def test_stream_order_without_waits(eng):
    """Five rounds of apply_updates -> process back to back with no wait in between - both staging sets are reused, the third call
    takes the first call's set - give what the same rounds give with engine.sync() after every call."""
    V, T, rounds = 2352, 2, 5
    n = V * T * 64
    outs = {}
    for waits in (False, True):
        g = make_voice(eng, V)
        g.reserve_updates(256)
        d_in = [eng.to_device(np.ascontiguousarray(gate_signal(V, 64 * T, 30 + r).reshape(V, T * 16, 4).transpose(1, 0, 2))) for r in range(rounds)]   # QUAD
        d_out = [eng.alloc(4 * n) for _ in range(rounds)]
        lists = [records(g, random_ops(V, 200, 40 + r)) for r in range(rounds)]
        eng.sync()
        for r in range(rounds):
            g.apply_updates(lists[r])
            if waits:
                eng.sync()
            g.process(T, [d_in[r]], [d_out[r]])
            if waits:
                eng.sync()
        outs[waits] = [d.download(np.float32, n).copy() for d in d_out] + [np.concatenate(list(read_tables(g).values()))]
        g.close()
    for r, (x, y) in enumerate(zip(outs[False], outs[True])):
        assert same(x, y), r
    assert np.abs(outs[False][rounds - 1]).max() > 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("V", SIZES)
def test_clear_some_voices(eng, V):
    """Three vectors, CLEAR(node = -1) on voices [64, 80), three more: those voices give a fresh graph's first three vectors on the
    same inputs, every other voice what an undisturbed run gives - outputs and every state word. The graph here is gated by its input:
    every clear() of it is a full reset. (With an ADSR that is not so - ADSR::clear() resets the segment only - and the yardstick is
    mlgpu_graph_clear at the same point: second part.)"""
    T, lo, hi = 3, 64, 80
    sig1, sig2 = {"gate": gate_signal(V, 64 * T, 50)}, {"gate": gate_signal(V, 64 * T, 51)}
    rest = np.r_[0:lo, hi:V]
    for adsr in (False, True):
        cleared, undisturbed, other = make_voice(eng, V, adsr), make_voice(eng, V, adsr), make_voice(eng, V, adsr)
        keys = rows_of(cleared)
        (y1,) = cleared.process_host(T, sig1)
        undisturbed.process_host(T, sig1)
        rec = [ml.Update.clear(-1, lo, hi - lo)]
        n_words = sum(1 for k in keys if k[0] == "s") - (7 if adsr else 0)
        assert cleared.update_device_records(rec) == n_words
        cleared.apply_updates(rec)
        if adsr:
            other.process_host(T, sig1)
            other.clear()          # mlgpu_graph_clear: every voice
        (yc,), (yu,), (yo,) = cleared.process_host(T, sig2), undisturbed.process_host(T, sig2), other.process_host(T, sig2)
        assert same(yc[lo:hi], yo[lo:hi]) and same(yc[rest], yu[rest]), adsr
        assert not same(yc[lo:hi], yu[lo:hi]) and np.abs(yc[lo:hi]).max() > 1e-4 and np.abs(y1[lo:hi]).max() > 1e-4
        tc, tu, to = read_tables(cleared, keys), read_tables(undisturbed, keys), read_tables(other, keys)
        for k in keys:
            assert same(tc[k][lo:hi], to[k][lo:hi]) and same(tc[k][rest], tu[k][rest]), (adsr, k)
        # one node: the glide's 67 words, the others' untouched
        one = [ml.Update.clear(cleared.ids["glide"], 0, 1)]
        assert cleared.update_device_records(one) == cleared.num_state("glide")
        cleared.apply_updates(one)
        t1 = read_tables(cleared, keys)
        small = make_voice(eng, 64, adsr)
        fresh = read_tables(small, [k for k in keys if k[1] == "glide" and k[0] == "s"])
        for k in keys:
            if k[0] == "s" and k[1] == "glide":
                assert t1[k][0] == fresh[k][0] and same(t1[k][1:], tc[k][1:]), k
            else:
                assert same(t1[k], tc[k]), k
        for g in (cleared, undisturbed, other, small):
            g.close()


@pytest.mark.gpu
def test_clear_refuses_delay_rings(eng):
    V = 80
    g = ml.Graph(eng, V)
    x = g.add("x", "input")
    d = g.add("d", "proc", Proc.INTEGER_DELAY, [x], max_delay=100.0)
    lp = g.add("lp", "proc", Proc.LOPASS, [d])
    g.add_output(lp)
    g.compile()
    g.clear()
    g.set_coeffs("lp", [float(c) for c in ml.Lopass.makeCoeffs(0.1, 0.7)])
    sig = {"x": lcg_noise(np.arange(V, dtype=np.uint32) + 9, 64)}
    g.process_host(1, sig)
    keys = rows_of(g)
    before = read_tables(g, keys)
    for rec in ([ml.Update.clear(d, 0, V)], [ml.Update.clear(-1, 64, 16)], [ml.Update.state(lp, 0, 0, V, 0), ml.Update.clear(d, 0, 1)]):
        with pytest.raises(ml.MlgpuError) as ei:
            g.apply_updates(rec)
        assert ei.value.status == Status.ERR_UNSUPPORTED and "rings" in str(ei.value) and "record %d of" % (len(rec) - 1) in str(ei.value)
        assert g.update_device_records(rec) == 0
    assert_tables_equal(read_tables(g, keys), before, "after the refusals")
    g.apply_updates([ml.Update.clear(lp, 64, 16)])       # its other nodes clear
    after = read_tables(g, keys)
    assert (after[("s", "lp", 0)][64:] == 0).all() and same(after[("s", "lp", 0)][:64], before[("s", "lp", 0)][:64]) and before[("s", "lp", 0)][64:].any()
    g.close()


@pytest.mark.gpu
def test_refusals_change_nothing(eng):
    """Every refusal of the list: status, a message naming the record's position, no table word changed - the good records before the
    bad one included."""
    V = 80
    g = make_voice(eng, V)
    ids = g.ids
    keys = rows_of(g)
    before = read_tables(g, keys)
    good = ml.Update.param(ids["pitch"], 0, V, 0.5)
    bad = [(ml.Update.param(ids["lp"], 0, 1, 0.0), Status.ERR_INVALID), (ml.Update.coeff(ids["pitch"], 0, 0, 1, 0.0), Status.ERR_INVALID),
           (ml.Update.state(ids["out"], 0, 0, 1, 0), Status.ERR_INVALID), (ml.Update.coeff(ids["fb"], 0, 0, 1, 0.0), Status.ERR_INVALID),
           (ml.Update.coeff(ids["lp"], g.L.mlgpu_graph_num_coeffs(g.h, ids["lp"]), 0, 1, 0.0), Status.ERR_RANGE), (ml.Update.state(ids["lp"], 2, 0, 1, 0), Status.ERR_RANGE),
           (ml.Update.state(ids["fb"], 64, 0, 1, 0), Status.ERR_RANGE), (ml.Update.param(ids["pitch"], V, 1, 0.0), Status.ERR_RANGE),
           (ml.Update.param(ids["pitch"], V - 1, 2, 0.0), Status.ERR_RANGE), (ml.Update.param(ids["pitch"], 5, 0, 0.0), Status.ERR_INVALID),
           (ml.Update.input_const(0, 1, 0.0), Status.ERR_INVALID), (ml.Update.param(len(ids) + 50, 0, 1, 0.0), Status.ERR_RANGE),
           (ml.Update(ids["pitch"], 9, 0, 0, 1, 0), Status.ERR_INVALID)]
    for rec, status in bad:
        with pytest.raises(ml.MlgpuError) as ei:
            g.apply_updates([good, rec, good])
        assert ei.value.status == status and "record 1 of 3" in str(ei.value), str(ei.value)
    assert_tables_equal(read_tables(g, keys), before, "after the refusals")
    g.apply_updates([])                                   # n == 0: fine, nothing happens
    assert g.L.mlgpu_graph_apply_updates(g.h, None, 0) == Status.OK
    not_compiled = ml.Graph(eng, V, voice_desc(), ["mix"], compile_now=False)
    with pytest.raises(ml.MlgpuError) as ei:
        not_compiled.apply_updates([good])
    assert ei.value.status == Status.ERR_INVALID and "compile first" in str(ei.value)
    not_compiled.compile_async()
    st = g.L.mlgpu_graph_apply_updates(not_compiled.h, (ml.Update * 1)(good), 1)   # while the job owns the graph (or just after)
    assert st == ml.BUSY
    while not not_compiled.compile_poll():
        pass
    not_compiled.apply_updates([good])
    assert (not_compiled.get_param("pitch") == 0.5).all()
    not_compiled.close()
    g.close()


@pytest.mark.gpu
def test_reserve(eng):
    """After reserve_updates(100) a list of 101 device records is ERR_RANGE and the tables are unchanged; 100 pass; a CLEAR counts
    its state words."""
    V = 2352
    g = make_voice(eng, V)
    keys = rows_of(g)
    assert staging(g) == ((None,) * 4, 0)
    g.reserve_updates(100)
    reserved = staging(g)
    assert all(reserved[0]) and reserved[1] == 100     # two sets of exactly what was asked for: apply must never replace them
    before = read_tables(g, keys)
    pitch = g.ids["pitch"]
    recs = [ml.Update.param(pitch, 7 * j, 7, 0.001 * (j + 1)) for j in range(101)]
    with pytest.raises(ml.MlgpuError) as ei:
        g.apply_updates(recs)
    assert ei.value.status == Status.ERR_RANGE and "101" in str(ei.value) and "100" in str(ei.value)
    assert_tables_equal(read_tables(g, keys), before, "after the refused list")
    clear_all = [ml.Update.clear(-1, 0, 16)]
    n_words = sum(1 for k in keys if k[0] == "s") - 7          # (ADSR::clear() resets one of its eight words)
    assert g.update_device_records(clear_all) == n_words > 100
    with pytest.raises(ml.MlgpuError) as ei:
        g.apply_updates(clear_all)
    assert ei.value.status == Status.ERR_RANGE
    some = [ml.Update.clear(g.ids["lp"], 0, 16)] + recs[:98]   # 2 + 98
    assert g.update_device_records(some) == 100
    assert_tables_equal(read_tables(g, keys), before, "after the refused CLEAR")
    assert staging(g) == reserved
    g.apply_updates(some)
    g.apply_updates(recs[:100])
    for j in range(4):                                         # both sets, more than once, small lists and full ones
        g.apply_updates(recs[:100] if j & 1 else recs[:1])
        assert staging(g) == reserved
    with pytest.raises(ml.MlgpuError) as ei:
        g.reserve_updates(2 ** 25 + 1)                         # more than one launch takes: refused at setup
    assert ei.value.status == Status.ERR_INVALID and staging(g) == reserved
    got = g.get_param("pitch").view(np.uint32)
    want = before[("p", "pitch", 0)].copy()
    for j in range(100):
        want[7 * j:7 * j + 7] = fbits(0.001 * (j + 1))
    assert same(got, want)
    g.close()


@pytest.mark.gpu
def test_recording(eng):
    """Refused while recording (the call reads host memory); applied between two launches of a recorded sequence it gives what two
    direct calls with the update in between give."""
    V, T = 80, 2
    n = V * T * 64
    gate = np.ascontiguousarray(gate_signal(V, 64 * T, 60).reshape(V, T * 16, 4).transpose(1, 0, 2))   # QUAD
    ops = coverage_ops(V) + random_ops(V, 40, 61)
    direct, recorded = make_voice(eng, V), make_voice(eng, V)
    d_in, d_a, d_b = eng.to_device(gate), eng.alloc(4 * n), eng.alloc(4 * n)
    keys = rows_of(recorded)
    before = read_tables(recorded, keys)
    with pytest.raises(ml.MlgpuError) as ei:
        with eng.record():
            recorded.apply_updates(records(recorded, ops))
    assert ei.value.status == Status.ERR_INVALID and "recording" in str(ei.value)
    assert_tables_equal(read_tables(recorded, keys), before, "after the refusal while recording")
    with eng.record() as seq:
        recorded.process(T, [d_in], [d_b])
    want, got = [], []
    for launch in range(2):
        direct.process(T, [d_in], [d_a])
        want.append(d_a.download(np.float32, n).copy())
        seq.launch()
        got.append(d_b.download(np.float32, n).copy())
        if launch == 0:
            direct.apply_updates(records(direct, ops))
            recorded.apply_updates(records(recorded, ops))
    assert same(got[0], want[0]) and same(got[1], want[1]) and not same(got[0], got[1])
    assert_tables_equal(read_tables(recorded, keys), read_tables(direct, keys), "after the second launch")
    seq.close()
    direct.close()
    recorded.close()


# ---- banks -----------------------------------------------------------------------------------------------------------------------
def make_bank(eng, which, V, tune=True):
    if which == "fused":
        b = eng.bank([Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN], V)
        assert b.fused and "cascade" not in b.kernel_name
    elif which == "cascade":
        b = eng.bank([Proc.HIPASS] * 4, V)
        assert b.fused and "cascade" in b.kernel_name
    else:
        eng.set_jit(False)
        try:
            b = eng.bank([Proc.NOISE_GEN, Proc.ONE_POLE], V)
        finally:
            eng.set_jit(True)
        assert not b.fused
    b.clear()
    if not tune:
        return b
    if which == "fused":
        b.set_coeffs(1, [float(c) for c in ml.Bandpass.makeCoeffs(0.1, 0.7)])
        b.set_coeff(2, 0, 0.25)
        b.set_input_const((55.0 * 2.0 ** (5.0 * np.arange(V) / V) / 48000.0).astype(np.float32))
    elif which == "cascade":
        for p in range(4):
            b.set_coeffs(p, [float(c) for c in ml.Hipass.makeCoeffs(0.02 + 0.01 * p, 0.9)])
    else:
        b.set_state(0, 0, np.arange(V, dtype=np.uint32) + 5)
        b.set_coeffs(1, [float(c) for c in ml.OnePole.makeCoeffs(0.1)])
    return b


def bank_ops(which, V, seed):
    """(kind, processor, index, first, n, bits) with 'i' for the input-const table: the coverage ranges, then 200 random records."""
    rng = np.random.default_rng(seed)
    ranges = coverage_ranges(V) + [(int(f), int(min(V - f, c))) for f, c in zip(rng.integers(0, V, 200), rng.integers(1, 21, 200))]
    ops = []
    for j, (first, n) in enumerate(ranges):
        special = [None, DENORMAL, NEG_ZERO, NAN_BITS][j] if j < 4 else None
        if which == "fused":
            c = ml.Bandpass.makeCoeffs(float(rng.uniform(0.02, 0.3)), float(rng.uniform(0.3, 1.2)))
            ops += [("c", 1, i, first, n, fbits(c[i])) for i in range(len(c))]
            ops += [("c", 2, 0, first, n, special if special is not None else fbits(rng.uniform(0.1, 0.5))),
                    ("s", 1, int(rng.integers(0, 2)), first, n, fbits(rng.uniform(-0.1, 0.1))), ("i", 0, 0, first, n, fbits(rng.uniform(0.001, 0.02)))]
        elif which == "cascade":
            p = int(rng.integers(0, 4))
            c = ml.Hipass.makeCoeffs(float(rng.uniform(0.01, 0.1)), float(rng.uniform(0.5, 1.2)))
            ops += [("c", p, i, first, n, fbits(c[i])) for i in range(len(c))]
            ops += [("s", int(rng.integers(0, 4)), int(rng.integers(0, 2)), first, n, special if special is not None else fbits(rng.uniform(-0.1, 0.1))),
                    ("i", 0, 0, first, n, fbits(0.5))]
        else:
            c = ml.OnePole.makeCoeffs(float(rng.uniform(0.01, 0.3)))
            ops += [("c", 1, i, first, n, fbits(c[i])) for i in range(len(c))]
            ops += [("s", 0, 0, first, n, int(rng.integers(1, 2 ** 32))),
                    ("s", 1, 0, first, n, special if special is not None else fbits(rng.uniform(-0.1, 0.1))), ("i", 0, 0, first, n, fbits(0.25))]
    return ops


def bank_tables(b):
    t = {("c", p, i): b.get_coeff(p, i).view(np.uint32).copy() for p in range(len(b.procs)) for i in range(b.num_coeffs(p))}
    t.update({("s", p, i): b.get_state(p, i).copy() for p in range(len(b.procs)) for i in range(b.num_state(p))})
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("V", SIZES)
@pytest.mark.parametrize("which", ["fused", "cascade", "unfused"])
def test_banks(eng, which, V):
    """A fused SawGen -> Bandpass -> Gain bank, an SVF cascade bank and a processor-by-processor bank: COEFF, STATE and INPUT_CONST
    records (and a CLEAR of some voices) against the row setters - get_coeff / get_state of every word and the outputs of two launches."""
    T = 2
    a, b = make_bank(eng, which, V), make_bank(eng, which, V)
    x = lcg_noise(np.arange(V, dtype=np.uint32) + 77, 64 * T) if which == "cascade" else None
    ya, yb = a.process_host(T, x), b.process_host(T, x)
    assert same(ya, yb)
    model = bank_tables(a)
    model[("i", 0, 0)] = np.zeros(V, np.uint32) if which != "fused" else (55.0 * 2.0 ** (5.0 * np.arange(V) / V) / 48000.0).astype(np.float32).view(np.uint32).copy()
    ops = bank_ops(which, V, 5)
    touched = model_apply(model, ops)
    # CLEAR of voices [64, 80): the words mlgpu_bank_clear writes, for those voices
    cleared = bank_tables(make_bank(eng, which, 64, tune=False))
    for k in [k for k in model if k[0] == "s"]:
        model[k][64:80] = cleared[k][0]
        if k not in touched:
            touched.append(k)
    for kind, p, i in touched:
        if kind == "c":
            a.set_coeff(p, i, model[(kind, p, i)].view(np.float32))
        elif kind == "s":
            a.set_state(p, i, model[(kind, p, i)])
        else:
            a.set_input_const(model[(kind, p, i)].view(np.float32))
    target = {"c": 1, "s": 2, "i": 3}
    recs = [ml.Update(p, target[kind], i, first, n, bits) for kind, p, i, first, n, bits in ops]
    recs.append(ml.Update.clear(-1, 64, 16))
    b.apply_updates(recs)
    tb = bank_tables(b)
    assert_tables_equal(tb, model, "as given", list(tb))
    for launch in range(2):
        ya, yb = a.process_host(T, x), b.process_host(T, x)
        assert same(ya, yb), launch
        assert_tables_equal(bank_tables(a), bank_tables(b), f"after launch {launch}")
    ok = np.isfinite(ya).all(1)
    assert ok.sum() > V // 2 and np.abs(ya[ok]).max() > 1e-4
    # a bank refuses what it has not: PARAM, a processor or slot that is not there, a range past the end
    before = bank_tables(b)
    for rec, status in ((ml.Update.param(0, 0, 1, 0.0), Status.ERR_INVALID), (ml.Update.coeff(len(b.procs), 0, 0, 1, 0.0), Status.ERR_RANGE),
                        (ml.Update.coeff(1, 7, 0, 1, 0.0), Status.ERR_RANGE), (ml.Update.input_const(V - 1, 2, 0.0), Status.ERR_RANGE)):
        with pytest.raises(ml.MlgpuError) as ei:
            b.apply_updates([recs[0], rec])
        assert ei.value.status == status and "record 1 of 2" in str(ei.value)
    b.reserve_updates(8)
    with pytest.raises(ml.MlgpuError) as ei:
        b.apply_updates(recs[:9])
    assert ei.value.status == Status.ERR_RANGE
    assert_tables_equal(bank_tables(b), before, "after the refusals")
    reserved = staging(b)
    assert all(reserved[0]) and reserved[1] >= 8
    for _ in range(5):                               # after a reserve: the same buffers, whatever their size, call after call
        b.apply_updates(recs[:8])
        assert staging(b) == reserved
    a.close()
    b.close()


@pytest.mark.gpu
def test_cpp_wrapper_apply_updates(tmp_path):
    """ml::gpu::VoiceBank::applyUpdates / reserveUpdates (include/mlgpu/mldsp_gpu.hpp): tests/cpp/param_updates_gpu_test.cpp, built
    here against the C ABI - a knob turned on some instruments of a resonator bank against coeffs() + commit()."""
    from madronalib_amd import _lib
    _lib.load()
    exe = str(tmp_path / "param_updates_gpu_test")
    lib = os.path.join(ROOT, "madronalib_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "param_updates_gpu_test.cpp"),
           "-o", exe, "-L" + lib, "-lmlgpu", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]
