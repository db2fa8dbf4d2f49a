"""Developer tool: what the launch boundary of the headline costs, measured before anything is built on it. Config 3's voices
(SawGen -> Bandpass -> Gain, parameters from cfg3_voice_params) in one process, two ways:
  (a) one V-voice bank on one engine: a step is L launches on one stream, every launch boundary a barrier across the chip;
  (b) the same voices as two V/2-voice banks on two engines (= two HIP streams) of the same device, launches issued alternately from
      this one host thread. Each half is serial on its own stream, the halves never meet: while one half's launch drains and its next
      is dispatched, the other half's wavefronts keep running.
  (c) (--serial) the two V/2-voice banks on ONE engine, launched alternately: the same two kernels per launch, serial on one stream.
      What (b) gains over (c) is the overlap; what (c) gains over (a) is the half-size launch by itself.
  (d) (--product) the V-voice bank on an engine whose launch parts are left at their default: the library's own two-part launch.
Every other engine here is set to one launch per call (Engine.set_launch_parts(1)), so (a), (b) and (c) are what they say; against a
library from before launch parts existed - the decision run of step 0 - there is nothing to set and (d) is not to be had.
  (--plan) three routes that cut the voices once more, into kernels of one wavefront per SIMD at config 3's size:
  (e) four V/4-voice banks on ONE engine, launched in turn: what a quarter-size launch costs by itself;
  (f) four V/4-voice banks on TWO engines, quarters 0 and 1 on the first and 2 and 3 on the second, issued q0, q2, q1, q3;
  (g) two V/4-voice banks on the first engine and one V/2-voice bank on the second, issued q0, half, q1: the first stream's kernel
      boundary falls in the middle of the second stream's kernel even when the streams start together.
The modes alternate ROUNDS times; each run is STEPS steps after WARMUP untimed ones, host wall clock from a sync of every engine to
the next sync of every engine. One JSON line per run on stdout; the verdict of the decision rule (every (b) below every (a) and the gap
between the ranges wider than (a)'s own range) on the last line, and with it the same rule for (f) and (g) against (d): a four-kernel
plan is built only if every run of it lies below every run of (d) by at least (d)'s own range.

  python tools/launch_parts_probe.py [--voices V] [--vectors T] [--launches L] [--steps N] [--warmup W] [--rounds R] [--serial] [--product] [--plan] [--only a|b|c|d|e|f|g]
                                      [--raw FILE]

`--only b --rounds 1` (or f, or g) is the shape to run under `rocprofv3 --kernel-trace` (a run of its own, no counters): the trace shows whether the
two halves' kernels overlap in time."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import madronalib_amd as ml  # noqa: E402
from madronalib_amd.constants import Layout, Proc  # noqa: E402
from madronalib_amd.sharding import cfg3_voice_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--voices", type=int, default=262144)
ap.add_argument("--vectors", type=int, default=30)
ap.add_argument("--launches", type=int, default=25)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--only", choices=["a", "b", "c", "d", "e", "f", "g"])
ap.add_argument("--serial", action="store_true", help="also run (c)")
ap.add_argument("--product", action="store_true", help="also run (d)")
ap.add_argument("--plan", action="store_true", help="also run (e), (f) and (g)")
ap.add_argument("--raw", help="append the JSON lines to this file as well")
args = ap.parse_args()
V, T, L = args.voices, args.vectors, args.launches
assert V % 4 == 0


def bank_of(eng, lo, hi):
    """Config 3's voices [lo, hi) of V as bench.py sets them up, with a ring of two output signals."""
    bank = eng.bank([Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN], hi - lo)
    bank.clear()
    freq, co = cfg3_voice_params(lo, hi, V, ml.Bandpass.makeCoeffs)
    for i in range(3):
        bank.set_coeff(1, i, co[i])
    bank.set_coeff(2, 0, 0.25)
    bank.set_input_const(freq)
    n = (hi - lo) * T * 64
    return bank, [eng.alloc(4 * n), eng.alloc(4 * n)]


engA = ml.Engine(0)
engines = {"a": [engA], "b": [ml.Engine(0), ml.Engine(0)]}
banks = {"a": [bank_of(engA, 0, V)],
         "b": [bank_of(engines["b"][0], 0, V // 2), bank_of(engines["b"][1], V // 2, V)]}
if args.serial or args.only == "c":
    engines["c"] = [engA]
    banks["c"] = [bank_of(engA, 0, V // 2), bank_of(engA, V // 2, V)]
HAS_PARTS = hasattr(ml.Engine, "set_launch_parts")
for es in engines.values():
    for e in es:
        if HAS_PARTS:
            e.set_launch_parts(1)
if args.product or args.only == "d":
    assert HAS_PARTS, "(d) needs a library with mlgpu_engine_set_launch_parts"
    engines["d"] = [ml.Engine(0)]
    banks["d"] = [bank_of(engines["d"][0], 0, V)]
Q = V // 4
if args.plan or args.only == "e":
    engines["e"] = [engA]
    banks["e"] = [bank_of(engA, q * Q, (q + 1) * Q) for q in range(4)]
if args.plan or args.only == "f":
    e0, e1 = engines["f"] = engines["b"]
    banks["f"] = [bank_of(e, q * Q, (q + 1) * Q) for e, q in ((e0, 0), (e1, 2), (e0, 1), (e1, 3))]
if args.plan or args.only == "g":
    e0, e1 = engines["g"] = engines["b"]
    banks["g"] = [bank_of(e0, 0, Q), bank_of(e1, V // 2, V), bank_of(e0, Q, 2 * Q)]
count = {m: 0 for m in banks}


def step(mode):
    for _ in range(L):
        k = count[mode] & 1
        for bank, outs in banks[mode]:
            bank.process(T, outs[k], Layout.QUAD)
        count[mode] += 1


def sync(mode):
    for e in engines[mode]:
        e.sync()


def run(mode):
    for _ in range(args.warmup):
        step(mode)
    sync(mode)
    engA.device_sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(mode)
    sync(mode)
    return (time.perf_counter() - t0) / args.steps * 1e3


name = engA.device_info()["name"]
results = {m: [] for m in banks}
raw = open(args.raw, "a") if args.raw else None
for r in range(args.rounds):
    for mode in banks:
        if args.only and mode != args.only:
            continue
        ms = run(mode)
        results[mode].append(ms)
        line = json.dumps({"round": r, "mode": mode, "banks": len(banks[mode]), "voices_per_bank": [b.V for b, _ in banks[mode]], "vectors": T,
                           "launches_per_step": L, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
                           "us_per_launch": ms * 1e3 / L, "device": name})
        print(line, flush=True)
        if raw:
            raw.write(line + "\n")
            raw.flush()

if results["a"] and results["b"]:
    a, b = results["a"], results["b"]
    gap, spread = min(a) - max(b), max(a) - min(a)
    verdict = {"a_ms": [min(a), float(np.median(a)), max(a)], "b_ms": [min(b), float(np.median(b)), max(b)],
               "gap_between_ranges_ms": gap, "a_range_ms": spread, "b_over_a_median": float(np.median(b) / np.median(a)),
               "build_the_rest": bool(gap > 0 and gap > spread)}
    for m in ("c", "d", "e", "f", "g"):
        if results.get(m):
            verdict[m + "_ms"] = [min(results[m]), float(np.median(results[m])), max(results[m])]
    d = results.get("d")
    for m in ("f", "g"):
        if d and results.get(m):
            gap_d, spread_d = min(d) - max(results[m]), max(d) - min(d)
            verdict[m + "_against_d"] = {"gap_between_ranges_ms": gap_d, "d_range_ms": spread_d,
                                         "median_over_d": float(np.median(results[m]) / np.median(d)),
                                         "build_it": bool(gap_d > 0 and gap_d >= spread_d)}
    line = json.dumps({"verdict": verdict})
    print(line, flush=True)
    if raw:
        raw.write(line + "\n")
if raw:
    raw.close()
for mode in banks:
    for bank, outs in banks[mode]:
        bank.close()
        for o in outs:
            o.free()
for e in engines["b"] + engines.get("d", []):
    e.close()
engA.close()
