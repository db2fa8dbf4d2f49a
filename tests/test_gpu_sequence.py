"""Recorded launch sequences (mlgpu_engine_begin_recording / mlgpu_sequence_launch, a hipGraph): a real-time block made of
several small launches replayed with one graph launch gives the same bits as the launches made one by one."""
import time

import numpy as np
import pytest

from madronalib_amd.constants import Layout, Op, Proc


@pytest.fixture(scope="module")
def eng():
    import madronalib_amd as ml
    e = ml.Engine(0)
    yield e
    e.close()


def make_block(eng, V, T):
    """One real-time block: three small banks, two elementwise ops, a mix to one channel. Returns (launch-all fn, objects)."""
    import madronalib_amd as ml
    n = V * T * 64
    saw = eng.bank([Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN], V)
    saw.clear()
    co = ml.Bandpass.makeCoeffs(0.1, 0.7)
    for i in range(3):
        saw.set_coeff(1, i, float(co[i]))
    saw.set_coeff(2, 0, 0.25)
    saw.set_input_const((55.0 * 2.0 ** (5.0 * np.arange(V) / V) / 48000.0).astype(np.float32))
    noise = eng.bank([Proc.NOISE_GEN, Proc.LOPASS], V)
    noise.set_state(0, 0, np.arange(V, dtype=np.uint32) + 5)
    noise.set_coeffs(1, ml.Lopass.makeCoeffs(0.05, 0.9))
    lfo = eng.bank([Proc.SINE_GEN], V)
    lfo.clear()
    lfo.set_input_const(np.full(V, 3.0 / 48000.0, np.float32))
    bufs = [eng.alloc(4 * n) for _ in range(5)]
    d_mix = eng.alloc(4 * T * 64)
    eng.mixdown_reserve(V, T)

    def block():
        saw.process(T, bufs[0], Layout.QUAD)
        noise.process(T, bufs[1], Layout.QUAD)
        lfo.process(T, bufs[2], Layout.QUAD)
        eng.op_apply(Op.MULTIPLY, bufs[1], bufs[2], None, bufs[3], n)
        eng.op_apply(Op.ADD, bufs[0], bufs[3], None, bufs[4], n)
        eng.mixdown(bufs[4], Layout.QUAD, V, T, d_mix)
    return block, d_mix, (saw, noise, lfo, bufs)


@pytest.mark.gpu
def test_sequence_replay_same_bits(eng):
    V, T, blocks = 4096, 1, 300
    blk_a, mix_a, keep_a = make_block(eng, V, T)
    blk_b, mix_b, keep_b = make_block(eng, V, T)
    # a: launches one by one
    outs_a = []
    for _ in range(6):
        blk_a()
        outs_a.append(mix_a.download(np.float32, T * 64).copy())
    # b: recorded once, replayed
    with eng.record() as seq:
        blk_b()
    assert seq.num_nodes >= 6
    outs_b = []
    for _ in range(6):
        seq.launch()
        outs_b.append(mix_b.download(np.float32, T * 64).copy())
    for a, b in zip(outs_a, outs_b):
        assert (a.view(np.uint32) == b.view(np.uint32)).all()
    assert np.abs(outs_a[-1]).max() > 0
    # cost per block (reported, not asserted: on ROCm 7.2 a graph launch of 7 kernel nodes is not cheaper than 7 launches):
    # throughput = many blocks back to back, latency = one block and wait
    def per_block(fn, wait_each):
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(blocks):
            fn()
            if wait_each:
                eng.sync()
        eng.sync()
        return (time.perf_counter() - t0) / blocks * 1e6
    res = {(name, w): per_block(fn, w) for name, fn in (("one by one", blk_a), ("sequence", seq.launch)) for w in (False, True)}
    print(f"\nblock of 7 kernels, {V} voices x {T} vector, us per block: back to back {res[('one by one', False)]:.1f} one by one / "
          f"{res[('sequence', False)]:.1f} recorded; launch + wait {res[('one by one', True)]:.1f} / {res[('sequence', True)]:.1f}")


@pytest.mark.gpu
def test_what_cannot_be_recorded(eng):
    import madronalib_amd as ml
    from madronalib_amd.constants import Region
    buf = eng.alloc(4 * 64 * 64)
    g = ml.Graph(eng, 64)
    g.add("x", "input")
    (rx,) = g.begin_region(Region.DOWNSAMPLE_2X, ["x"])
    y = g.end_region(rx, "y")
    g.add_output(y)
    g.compile()
    ev = ml.Events(eng, 4, 4)
    with pytest.raises(ml.MlgpuError):
        with eng.record():
            buf.upload(np.zeros(64 * 64, np.float32))          # waits for the device
    with pytest.raises(ml.MlgpuError):
        with eng.record():
            g.process(1, [buf], [buf])                          # counts DSPVectors
    with pytest.raises(ml.MlgpuError):
        with eng.record():
            ev.process(1, 0, [buf] + [None] * 7)                # host work per call
    with eng.record() as seq:                                   # and the engine still records after the refusals
        eng.op_apply(Op.ADD, buf, buf, None, buf, 64 * 64)
    seq.launch()
    eng.sync()


def _reader(eng, kind, V=256):
    """An object of `kind` and a launch that reads its device memory into `out` (n floats), the same bits every time it replays."""
    import madronalib_amd as ml
    n = V * 64
    out = eng.alloc(4 * 2 * n)
    x = eng.alloc(4 * n).upload(np.sin(np.arange(n, dtype=np.float32) * 0.01).astype(np.float32))
    if kind == "bank":
        obj = eng.bank([Proc.GAIN], V)
        obj.set_coeff(0, 0, 0.5)
        obj.set_input_const(np.linspace(0.1, 1.0, V, dtype=np.float32))
        return obj, lambda: obj.process(1, out), out, n
    if kind == "graph":
        obj = ml.Graph(eng, V, [dict(name="x", type="input"), dict(name="p", type="param"),
                                dict(name="y", type="op", kind=Op.MULTIPLY, inputs=["x", "p"])], ["y"])
        obj.set_param("p", np.linspace(0.5, 2.0, V, dtype=np.float32))
        return obj, lambda: obj.process(1, [x], [out]), out, n
    if kind == "resampler":
        obj = ml.Resampler(eng, V, 1, True)

        def launch():
            obj.clear()                       # every replay starts from the same filter state
            obj.process(1, x, out)
        return obj, launch, out, 2 * n
    assert kind == "transport"
    obj = ml.Transport(eng, 4, 2)
    obj.update_time(0.0, 120.0, True, 48000.0)
    obj.process_host(2)                       # the beat-phase signal a recorded launch reads
    m = 4 * 64 * 2

    def launch():                             # the C call: Engine.op_apply takes buffer objects, not the beat-phase pointer
        assert eng.L.mlgpu_op_apply(eng.h, Op.ABS, obj.beat_phase, None, None, out.ptr, m) == ml.Status.OK
    return obj, launch, out, m


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bank", "graph", "resampler", "transport"])
def test_destroy_under_a_live_sequence(eng, kind):
    """An object destroyed while a recorded sequence that reads it lives is gone for its owner at once; its device memory stays
    until the last sequence goes, so the sequence replays the same bits."""
    import madronalib_amd as ml
    obj, launch, out, n = _reader(eng, kind)
    with eng.record() as seq:
        launch()
    try:
        seq.launch()
        first = out.download(np.float32, n)
        assert np.abs(first).max() > 0
        assert getattr(obj.L, obj._destroy)(obj.h) == ml.Status.OK
        obj.h = None
        # memory freed by the destroy would be handed out again here
        junk = [eng.alloc(4 * n).upload(np.full(n, np.nan, np.float32)) for _ in range(8)]
        out.upload(np.zeros(n, np.float32))
        seq.launch()
        again = out.download(np.float32, n)
        assert (again.view(np.uint32) == first.view(np.uint32)).all()
        for j in junk:
            j.free()
    finally:
        seq.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bank", "graph", "events", "transport", "published_signal", "resampler", "process_buffer"])
def test_destroy_while_recording_is_refused(eng, kind):
    """Destroying waits for the device, which would invalidate the capture: every handle refuses while its engine records, the
    recording still gives a sequence that launches, and the object stays usable."""
    import madronalib_amd as ml
    V = 64
    a, b = eng.alloc(4 * V * 64), eng.alloc(4 * V * 64 * 2)
    make, use = {
        "bank": (lambda: eng.bank([Proc.GAIN], V), lambda o: o.process_host(1)),
        "graph": (lambda: ml.Graph(eng, V, [dict(name="x", type="input"), dict(name="y", type="op", kind=Op.ADD, inputs=["x", "x"])], ["y"]),
                  lambda o: o.process(1, [a], [b])),
        "events": (lambda: ml.Events(eng, 4, 2), lambda o: o.process_host(1)),
        "transport": (lambda: ml.Transport(eng, 4, 2), lambda o: o.process_host(1)),
        "published_signal": (lambda: ml.PublishedSignal(eng, 256, 4, 1, 0), lambda o: o.write(1, [a], V, 0, 4)),
        "resampler": (lambda: ml.Resampler(eng, V, 1, True), lambda o: o.process(1, a, b)),
        "process_buffer": (lambda: ml.ProcessBuffer(eng, 1, 1, 64), lambda o: o.process([np.zeros(64, np.float32)], 64, lambda *_: None)),
    }[kind]
    obj = make()
    with eng.record() as seq:
        eng.op_apply(Op.ADD, a, a, None, a, V * 64)
        st = getattr(obj.L, obj._destroy)(obj.h)
        msg = eng.L.mlgpu_last_error(eng.h).decode()
    assert st == ml.Status.ERR_INVALID and "not while recording" in msg
    seq.launch()
    eng.sync()
    seq.close()
    use(obj)
    eng.sync()
    obj.close()
