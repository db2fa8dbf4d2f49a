"""The rule of voice tails (include/mlgpu.h, VOICE TAILS) restated in Python sets, for tests/test_voice_tails_cpu.py and
tests/test_gpu_voice_tails.py. It keeps every list ever made and takes results in literally as the header says; it shares no code
and no trick with madronalib_amd/csrc/voice_tails.cpp."""
import numpy as np


def loud_bits(peaks, quiet_bits):
    """[K] uint32 peaks -> [K] bool: strictly above the threshold, as unsigned integers."""
    return np.asarray(peaks, np.uint32).astype(np.uint64) > np.uint64(quiet_bits)


class Rule:
    def __init__(self, hold=1):
        self.hold = int(hold)
        self.lists = []          # lists[j - 1]: dict(L, S, noted, vectors, loud) of L_j
        self.c = 0               # the last launch taken in
        self.quiet = {}          # voice -> quiet DSPVectors behind it (absent: 0)
        self.quiet_behind = {}   # voice -> quiet[v] at the moment a next_list dropped it

    def _take_in(self, upto):
        while self.c < upto:
            l = self.lists[self.c]
            for i, v in enumerate(l["L"]):
                if v in l["S"] or (l["noted"] and l["loud"][i]):
                    self.quiet[v] = 0
                elif l["noted"]:
                    self.quiet[v] = self.quiet.get(v, 0) + l["vectors"]
            self.c += 1

    def next_list(self, must, taken_in=None):
        """L_m+1 for the must-set, with the launches up to `taken_in` taken in (None: every one there is)."""
        m = len(self.lists)
        self._take_in(m if taken_in is None else max(self.c, min(int(taken_in), m)))
        must = [int(v) for v in must]
        keep = set(must)
        if self.lists:
            for v in self.lists[-1]["L"]:
                if self.quiet.get(v, 0) < self.hold or any(v in self.lists[j]["S"] for j in range(self.c, m)):
                    keep.add(v)
                elif v not in keep:
                    self.quiet_behind[v] = self.quiet.get(v, 0)
        L = sorted(keep)
        self.lists.append(dict(L=L, S=set(must), noted=False, vectors=0, loud=None))
        return np.array(L, np.uint32)

    def note(self, n_vectors, loud):
        l = self.lists[-1]
        assert not l["noted"] and len(loud) == len(l["L"])
        l.update(noted=True, vectors=int(n_vectors), loud=[bool(b) for b in loud])
