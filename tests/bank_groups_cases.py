"""Expected values and cases of mlgpu_bank_process_groups (a fused bank whose voices come in groups of adjacent voices), shared by
tests/test_bank_groups_cpu.py and tests/test_gpu_bank_groups.py."""
import numpy as np

from madronalib_amd.constants import Op, Proc

GROUP_SIZES = (1, 2, 4, 8, 16)
T = 3  # DSPVectors per case: one launch of 3, or launches of 1 + 2
# voice counts: one full wavefront and a quarter of one (dead lanes, dead groups); nine full 256-voice workgroups (eight of them
# through the XCD remap, one not) and a last one of 48 voices
VOICES = (80, 2352)


def expected_group_sums(oracle, voices, group, gains=None, flush=False):
    """voices [V][S] float32, the per-voice signals the CPU checker gives -> [V / group][S]: each voice times its gain in float32
    (gains None: no multiply), then ((0 + y[cG]) + y[cG + 1]) + ... + y[cG + G - 1] in voice order with float32 adds, every operation
    under the checker's flush-denormals mode when `flush`. group 1 is the voices themselves (the kernel's plain store: no add)."""
    y = np.ascontiguousarray(voices, np.float32)
    V, S = y.shape
    assert V % group == 0
    with oracle.flush_denormals(flush):
        if gains is not None:
            g = np.ascontiguousarray(np.repeat(np.asarray(gains, np.float32)[:, None], S, axis=1))
            y = oracle.op_f32(Op.MULTIPLY, y, g)
        if group == 1:
            return y
        ys = y.reshape(V // group, group, S)
        acc = np.zeros((V // group, S), np.float32)
        for p in range(group):
            acc = oracle.op_f32(Op.ADD, acc, np.ascontiguousarray(ys[:, p]))
    return acc


def special_gains(V, seed=3):
    """Per-voice gains in (-1, 1) with a -0.0, a 0.0 and a denormal among them - in the first group and again in the last voices."""
    g = np.random.default_rng(seed + V).uniform(-1, 1, V).astype(np.float32)
    for base in (0, V - 16):
        g[base + 1] = np.float32(-0.0)
        g[base + 2] = np.float32(0.0)
        g[base + 5] = np.float32(1e-40)
    return g


class Chain:
    """One of the three kernel shapes: procs, coefficients [NC][V], the per-voice constant input or the streamed one."""

    def __init__(self, name, oracle, V, in_group=1):
        self.name, self.V, self.in_group = name, V, in_group
        self.in_const = self.in_rows = None
        rng = np.random.default_rng(V + len(name))
        few = np.stack([oracle.make_coeffs("bandpass", 0.02 + 0.3 * j / 16, 0.6) for j in range(16)], 1)  # [3][16]
        bandpass = np.ascontiguousarray(few[:, (np.arange(V) * 7) % 16])
        if name in ("saw", "saw_odd"):
            # SawGen -> Bandpass -> Gain on a per-voice constant frequency: no signal, the fast head; saw_odd: a frequency below 2^-64
            # in one lane of the first wavefront and one of the last, whose wavefronts then take the slow head
            self.procs = [Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN]
            self.coeffs = np.ascontiguousarray(np.concatenate([bandpass, np.full((1, V), 0.25, np.float32)], 0))
            self.in_const = (55.0 * 2.0 ** (5.0 * rng.random(V)) / 48000.0).astype(np.float32)
            if name == "saw_odd":
                self.in_const[[5, V - 3]] = np.float32(1e-30)
        elif name == "bandpass":
            # Bandpass alone on a streamed input of V / in_group rows: HAS_SIGNAL, the input group
            from inputs import lcg_noise
            self.procs = [Proc.BANDPASS]
            self.coeffs = bandpass
            self.in_rows = lcg_noise(np.arange(V // in_group, dtype=np.uint32) + 29, 64 * T)
        elif name == "impulse":
            # ImpulseGen: its table in LDS (and the workgroup barrier after staging it) beside the strip
            self.procs = [Proc.IMPULSE_GEN]
            self.coeffs = np.zeros((0, V), np.float32)
            self.in_const = (0.01 + 0.2 * rng.random(V)).astype(np.float32)
        else:
            raise ValueError(name)

    def oracle_voices(self, oracle, flush=False):
        """([V][64 T] per-voice signals, final state) from the CPU checker: the streamed rows expanded to one per voice."""
        st = oracle.chain_clear(self.procs, self.V)
        x = None if self.in_rows is None else np.ascontiguousarray(np.repeat(self.in_rows, self.in_group, axis=0))
        with oracle.flush_denormals(flush):
            y = oracle.chain_process(self.procs, T, self.coeffs, st, x, self.in_const, n_threads=4)
        return y, st
