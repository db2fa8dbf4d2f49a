// The host half of voice tails (madronalib_amd/csrc/voice_tails.cpp) without a device: built by g++ from voice_tails.cpp and
// voice_list.cpp alone - once plainly, once under the address and undefined-behaviour sanitizers - by tests/test_voice_tails_cpu.py.
// A fake Api stands in for the device: its "launch" works the loud bits out of peaks in host memory, its events complete when the test
// says so (in order, as a stream's do), a result's words are garbage until then, and it counts the queries and the waits.
// The rule of include/mlgpu.h (VOICE TAILS) is restated here as a brute-force model over std::set, which keeps every list that was
// ever made and takes results in literally as the header says; the object has to agree with it list by list.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <set>
#include <vector>

#include "../../madronalib_amd/csrc/voice_tails.hpp"

namespace
{
int failures = 0;
#define CHECK(cond)                                              \
  do                                                             \
  {                                                              \
    if (!(cond))                                                 \
    {                                                            \
      if (++failures < 30) printf("FAILED line %d: %s\n", __LINE__, #cond); \
    }                                                            \
  } while (0)

using Set = std::set<uint32_t>;
using List = std::vector<uint32_t>;

// ---- the fake device ----
struct Fake
{
  struct Event
  {
    bool complete{true};
  };
  struct InFlight
  {
    Event* ev;
    unsigned slot;
    std::vector<uint64_t> bits;
  };
  unsigned depth;
  size_t words;
  std::vector<std::vector<uint64_t>> slotWords;
  const uint64_t* ptrs[mltail::kMaxDepth]{};
  std::deque<InFlight> flying;
  std::vector<uint64_t> staged;
  unsigned stagedSlot{0};
  int creates{0}, destroys{0}, launches{0}, records{0}, queries{0}, waits{0};
  bool failQuery{false};

  Fake(unsigned depth_, size_t maxListed) : depth(depth_), words((maxListed + 63) / 64), slotWords(depth_, std::vector<uint64_t>((maxListed + 63) / 64, 0))
  {
    for (unsigned s = 0; s < depth; ++s) ptrs[s] = slotWords[s].data();
  }
  void deliverFront()
  {
    InFlight& f = flying.front();
    for (size_t w = 0; w < f.bits.size(); ++w) slotWords[f.slot][w] = f.bits[w];
    f.ev->complete = true;
    flying.pop_front();
  }
  void complete(size_t n)  // the n oldest results arrive
  {
    while (n-- > 0 && !flying.empty()) deliverFront();
  }
  mltail::Api api()
  {
    mltail::Api a;
    a.ctx = this;
    a.create = [](void* c, void** ev) {
      ++((Fake*)c)->creates;
      *ev = new Event();
      return true;
    };
    a.destroy = [](void* c, void* ev) {
      ++((Fake*)c)->destroys;
      delete (Event*)ev;
    };
    a.launch = [](void* c, unsigned slot, const uint32_t* peak, size_t K, uint32_t quietBits) {
      Fake* f = (Fake*)c;
      ++f->launches;
      if (slot >= f->depth || K == 0 || (K + 63) / 64 > f->words) return false;
      f->staged.assign((K + 63) / 64, 0);
      for (size_t i = 0; i < K; ++i)
        if (peak[i] > quietBits) f->staged[i >> 6] |= (uint64_t)1 << (i & 63);
      f->stagedSlot = slot;
      // until the result arrives the slot's words hold the opposite of it: reading them early shows
      for (size_t w = 0; w < f->words; ++w) f->slotWords[slot][w] = w < f->staged.size() ? ~f->staged[w] : ~(uint64_t)0;
      return true;
    };
    a.record = [](void* c, void* ev) {
      Fake* f = (Fake*)c;
      ++f->records;
      ((Event*)ev)->complete = false;
      f->flying.push_back(InFlight{(Event*)ev, f->stagedSlot, f->staged});
      return true;
    };
    a.query = [](void* c, void* ev) {
      Fake* f = (Fake*)c;
      ++f->queries;
      if (f->failQuery) return -1;
      return ((Event*)ev)->complete ? 1 : 0;
    };
    a.wait = [](void* c, void* ev) {
      Fake* f = (Fake*)c;
      ++f->waits;
      while (!((Event*)ev)->complete && !f->flying.empty()) f->deliverFront();
      return ((Event*)ev)->complete;
    };
    return a;
  }
};

// ---- the rule, restated ----
struct Model
{
  struct Made
  {
    Set L, S, loud;
    bool awaiting{true}, noted{false}, complete{false};
    uint64_t vectors{0};
  };
  size_t nVoices, maxListed;
  unsigned depth;
  std::vector<Made> lists;  // lists[j - 1] is L_j
  size_t c{0};
  std::vector<uint64_t> quiet;
  uint32_t quietBits{0x38d1b717u};
  uint64_t hold{1};

  Model(size_t V, size_t maxL, unsigned d) : nVoices(V), maxListed(maxL), depth(d), quiet(V, 0) {}
  size_t outstanding() const  // noted, with something to ask the device, not taken in
  {
    size_t n = 0;
    for (size_t j = c; j < lists.size(); ++j) n += (lists[j].noted && !lists[j].L.empty()) ? 1 : 0;
    return n;
  }
  void arrive(size_t n)  // the n oldest results that are still out
  {
    for (size_t j = c; j < lists.size() && n > 0; ++j)
      if (lists[j].noted && !lists[j].complete)
      {
        lists[j].complete = true;
        --n;
      }
  }
  void takeIn(bool all)
  {
    while (c < lists.size())
    {
      Made& l = lists[c];
      if (l.awaiting) break;
      if (l.noted && !l.complete && !all) break;
      for (uint32_t v : l.L)
      {
        if (l.S.count(v) || (l.noted && l.loud.count(v)))
          quiet[v] = 0;
        else if (l.noted)
          quiet[v] += l.vectors;
      }
      ++c;
    }
  }
  static int validate(const List& must, size_t V)
  {
    for (size_t i = 0; i < must.size(); ++i)
    {
      if (i > 0 && must[i] <= must[i - 1]) return MLGPU_ERR_INVALID;
      if (must[i] >= V) return MLGPU_ERR_RANGE;
    }
    return MLGPU_OK;
  }
  int nextList(const List& must, size_t capacity, List& out, size_t& n)
  {
    n = 0;
    const int vst = validate(must, nVoices);
    if (vst != MLGPU_OK) return vst;
    takeIn(false);
    Set next(must.begin(), must.end());
    if (!lists.empty())
      for (uint32_t v : lists.back().L)
      {
        bool keep = quiet[v] < hold;
        for (size_t j = c; j < lists.size() && !keep; ++j) keep = lists[j].S.count(v) != 0;  // (lists[j] is L_j+1: c < j + 1 <= m)
        if (keep) next.insert(v);
      }
    n = next.size();
    if (n > capacity || n > maxListed) return MLGPU_ERR_RANGE;
    if (!lists.empty()) lists.back().awaiting = false;
    Made m;
    m.L = next;
    m.S = Set(must.begin(), must.end());
    lists.push_back(m);
    out.assign(next.begin(), next.end());
    return MLGPU_OK;
  }
  int note(uint64_t vectors, const uint32_t* peak)
  {
    if (lists.empty() || !lists.back().awaiting) return MLGPU_ERR_INVALID;
    if (!peak) return MLGPU_ERR_INVALID;
    Made& l = lists.back();
    l.awaiting = false;
    if (l.L.empty())
    {
      l.noted = l.complete = true;
      return MLGPU_OK;
    }
    if (outstanding() == depth) return MLGPU_ERR_BUSY;
    l.noted = true;
    l.vectors = vectors;
    size_t i = 0;
    for (uint32_t v : l.L)
      if (peak[i++] > quietBits) l.loud.insert(v);
    return MLGPU_OK;
  }
  void wait() { takeIn(true); }
  void clear()
  {
    lists.clear();
    c = 0;
    quiet.assign(nVoices, 0);
  }
};

struct Rig
{
  Fake fake;
  mltail::Tails tails;
  Rig(size_t V, size_t maxListed, unsigned depth) : fake(depth, maxListed < V ? maxListed : V)
  {
    CHECK(tails.init(V, maxListed, depth, fake.api(), fake.ptrs) == MLGPU_OK);
  }
  List next(const List& must, int want = MLGPU_OK, size_t capacity = 100000)
  {
    List out(capacity < 4096 ? capacity : 4096, 0xdeadbeefu);
    size_t n = 0;
    const int waits = fake.waits;
    const int st = tails.nextList(must.empty() ? nullptr : must.data(), must.size(), out.data(), out.size(), &n);
    CHECK(fake.waits == waits);
    CHECK(st == want);
    lastN = n;
    out.resize(st == MLGPU_OK ? n : 0);
    return out;
  }
  int note(size_t vectors, const List& peaks)
  {
    const int waits = fake.waits, queries = fake.queries;
    static const uint32_t none = 0;
    const int st = tails.note(vectors, peaks.empty() ? &none : peaks.data());
    CHECK(fake.waits == waits && fake.queries == queries);
    return st;
  }
  size_t lastN{0};
};

const uint32_t Q = 0x38d1b717u;  // the threshold the object starts with

// ---- hand-written cases ----
void thresholdIsStrict()
{
  Rig r(16, 16, 2);
  CHECK(r.tails.setThreshold(1000, 1) == MLGPU_OK);
  CHECK(r.next({1, 3, 5, 7, 9}) == List({1, 3, 5, 7, 9}));
  CHECK(r.note(1, {0, 999, 1000, 1001, 0x7fc00000u}) == MLGPU_OK);
  r.fake.complete(1);
  CHECK(r.next({}) == List({1, 3, 5, 7, 9}));  // all of S_1: reset whatever the peaks
  CHECK(r.note(1, {0, 999, 1000, 1001, 0x7fc00000u}) == MLGPU_OK);
  r.fake.complete(1);
  CHECK(r.next({}) == List({7, 9}));  // > 1000 only: 1001 and the NaN
  CHECK(r.fake.launches == 2 && r.fake.records == 2);
}

void holdReachedExactly()
{
  Rig r(8, 8, 4);
  CHECK(r.tails.setThreshold(Q, 0) == MLGPU_ERR_INVALID);
  CHECK(r.tails.setThreshold(Q, 5) == MLGPU_OK);
  CHECK(r.next({2}) == List({2}));
  CHECK(r.note(7, {0}) == MLGPU_OK);  // in the must-set: the 7 quiet vectors do not count
  r.fake.complete(1);
  CHECK(r.next({}) == List({2}));
  CHECK(r.note(2, {0}) == MLGPU_OK);  // quiet 2
  r.fake.complete(1);
  CHECK(r.next({}) == List({2}));
  CHECK(r.note(2, {Q}) == MLGPU_OK);  // quiet 4 (the threshold itself is quiet)
  r.fake.complete(1);
  CHECK(r.next({}) == List({2}));
  CHECK(r.note(1, {0}) == MLGPU_OK);  // quiet 5: the hold, reached exactly
  r.fake.complete(1);
  CHECK(r.next({}) == List({}));
  CHECK(r.note(1, {}) == MLGPU_OK && r.tails.pending() == 0);  // an empty list: nothing launched, complete at once
  CHECK(r.fake.launches == 4);
}

void resets()
{
  Rig r(8, 8, 4);
  r.tails.setThreshold(Q, 3);
  auto block = [&](const List& must, size_t vectors, const List& peaks) {
    List l = r.next(must);
    CHECK(r.note(vectors, peaks) == MLGPU_OK);
    r.fake.complete(1);
    return l;
  };
  CHECK(block({4}, 1, {0}) == List({4}));
  CHECK(block({}, 2, {0}) == List({4}));       // quiet 2
  CHECK(block({}, 1, {Q + 1}) == List({4}));   // loud: quiet 0
  CHECK(block({}, 2, {0}) == List({4}));       // quiet 2
  CHECK(block({4}, 1, {0}) == List({4}));      // a must-set: quiet 0 (a retrigger, silent so far)
  CHECK(block({}, 2, {0}) == List({4}));       // quiet 2
  CHECK(block({}, 1, {0}) == List({4}));       // quiet 3: listed once more (this launch reached the hold) ...
  CHECK(r.next({}) == List({}));               // ... and gone
}

void unNotedAndLate()
{
  Rig r(8, 8, 4);
  r.tails.setThreshold(Q, 1);
  CHECK(r.next({1, 2}) == List({1, 2}));
  CHECK(r.note(1, {0, 0}) == MLGPU_OK);
  // nothing has arrived: both stay through S_1 (c = 0 < 1), and L_2 goes without a note
  CHECK(r.next({}) == List({1, 2}));
  CHECK(r.tails.pending() == 1);
  CHECK(r.next({2}) == List({1, 2}));  // L_3, S_3 = {2}
  CHECK(r.note(1, {0, 0}) == MLGPU_OK);
  CHECK(r.note(1, {0, 0}) == MLGPU_ERR_INVALID);  // one note per list
  r.fake.complete(1);  // launch 1 arrives: quiet[1] = quiet[2] = 0 (both in S_1); L_2 un-noted: taken in with it; c = 2
  CHECK(r.next({}) == List({1, 2}));  // L_4: 1 by quiet 0 < 1, 2 by S_3
  CHECK(r.note(1, {0, 0}) == MLGPU_OK);
  r.fake.complete(1);  // launch 3: 1 quiet -> 1, 2 in S_3 -> 0
  CHECK(r.next({}) == List({2}));  // L_5 (launch 4 still out: 1 is dropped on what is known, 2 kept)
  r.fake.complete(1);  // launch 4: 1 -> 2, 2 -> 1
  CHECK(r.next({}) == List({}));
  CHECK(r.tails.pending() == 0);
  // a note before any list, and after clear
  Rig s(8, 8, 1);
  CHECK(s.note(1, {0}) == MLGPU_ERR_INVALID);
  CHECK(s.next({3}) == List({3}));
  CHECK(s.tails.note(1, nullptr) == MLGPU_ERR_INVALID);
  CHECK(s.tails.note(1, (const uint32_t*)(uintptr_t)0x1002) == MLGPU_ERR_INVALID);
  CHECK(s.note(1, {0}) == MLGPU_OK);  // the refusals left the list waiting
}

void busyAtDepth()
{
  Rig r(8, 8, 2);
  r.tails.setThreshold(Q, 1);
  CHECK(r.next({0, 5}) == List({0, 5}));
  CHECK(r.note(1, {0, 0}) == MLGPU_OK);
  CHECK(r.next({}) == List({0, 5}));
  CHECK(r.note(1, {0, 0}) == MLGPU_OK);
  CHECK(r.next({}) == List({0, 5}));
  const int launches = r.fake.launches, records = r.fake.records;
  CHECK(r.note(1, {0, 0}) == MLGPU_ERR_BUSY);  // two are outstanding: nothing enqueued, L_3 goes without peaks
  CHECK(r.fake.launches == launches && r.fake.records == records && r.tails.pending() == 2);
  CHECK(r.note(1, {0, 0}) == MLGPU_ERR_INVALID);
  r.fake.complete(2);  // launch 1: in S_1, 0. launch 2: quiet 1. L_3: no peaks
  CHECK(r.next({}) == List({}));
  CHECK(r.tails.pending() == 0);
}

void clearForgets()
{
  Rig r(8, 8, 2);
  r.tails.setThreshold(Q, 2);
  CHECK(r.next({1, 6}) == List({1, 6}));
  CHECK(r.note(1, {0, 0}) == MLGPU_OK);
  r.tails.clear();
  CHECK(r.tails.pending() == 0);
  CHECK(r.note(1, {0, 0}) == MLGPU_ERR_INVALID);
  CHECK(r.next({}) == List({}));
  r.fake.complete(8);
  CHECK(r.next({6}) == List({6}));
  CHECK(r.note(1, {0}) == MLGPU_OK);
  r.fake.complete(8);
  CHECK(r.next({}) == List({6}));
}

void refusalsLeaveTheStateIntact()
{
  Rig r(100, 4, 2);
  r.tails.setThreshold(Q, 1);
  CHECK(r.tails.maxListed() == 4);
  CHECK(r.next({10, 20, 30}) == List({10, 20, 30}));
  CHECK(r.note(1, {Q + 5, Q + 5, 0}) == MLGPU_OK);
  r.fake.complete(1);
  // every refusal of a must-set: nothing is made, numbered or taken in
  const int queries = r.fake.queries;
  r.next({5, 5}, MLGPU_ERR_INVALID);
  r.next({7, 6}, MLGPU_ERR_INVALID);
  r.next({1, 2, 100}, MLGPU_ERR_RANGE);
  r.next({0xffffffffu}, MLGPU_ERR_RANGE);
  r.next({3, 2, 100}, MLGPU_ERR_INVALID);  // the first fault found is the answer
  size_t n = 77;
  uint32_t out[4];
  CHECK(r.tails.nextList(nullptr, 2, out, 4, &n) == MLGPU_ERR_INVALID);
  CHECK(r.fake.queries == queries && r.tails.pending() == 1);
  // too long for max_listed, then for the capacity: *n says how long, and the repeat with room is the list
  r.next({1, 2}, MLGPU_ERR_RANGE);  // 1 2 10 20 30 (30 is still there: S_1)
  CHECK(r.lastN == 5);
  r.next({1}, MLGPU_ERR_RANGE, 3);
  CHECK(r.lastN == 4);
  CHECK(r.note(1, {0, 0, 0}) == MLGPU_ERR_INVALID);  // (L_1 was noted; no new list was made)
  CHECK(r.next({1}) == List({1, 10, 20, 30}));
  CHECK(r.note(1, {0, Q + 1, 0, 0}) == MLGPU_OK);
  r.fake.complete(1);
  CHECK(r.next({}) == List({1, 10}));
  // a query that fails is reported, and nothing is lost
  CHECK(r.note(1, {Q + 1, 0}) == MLGPU_OK);
  r.fake.failQuery = true;
  r.next({}, MLGPU_ERR_HIP);
  r.fake.failQuery = false;
  r.fake.complete(1);
  CHECK(r.next({}) == List({1}));
}

void setupRefusals()
{
  Fake f(2, 8);
  mltail::Tails t;
  CHECK(t.init(0, 8, 2, f.api(), f.ptrs) == MLGPU_ERR_INVALID);
  CHECK(t.init(8, 0, 2, f.api(), f.ptrs) == MLGPU_ERR_INVALID);
  CHECK(t.init(8, 8, 0, f.api(), f.ptrs) == MLGPU_ERR_INVALID);
  CHECK(t.init(8, 8, 9, f.api(), f.ptrs) == MLGPU_ERR_INVALID);
  size_t n;
  uint32_t out[1];
  CHECK(t.nextList(nullptr, 0, out, 1, &n) == MLGPU_ERR_INVALID);  // not set up
  CHECK(t.init(8, 8, 2, f.api(), f.ptrs) == MLGPU_OK && f.creates == 2);
  CHECK(t.init(8, 8, 2, f.api(), f.ptrs) == MLGPU_ERR_INVALID);
}

// ---- the random walk ----
struct Rng
{
  uint64_t s;
  uint32_t next()
  {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  uint32_t below(uint32_t n) { return next() % n; }
};

// a voice's peak in launch j: a function of the two alone, so that an object that runs later or earlier sees the same voice do the same
uint32_t peakOf(uint32_t v, uint64_t launch, uint32_t quietBits)
{
  uint64_t h = (v * 0x9e3779b97f4a7c15ull) ^ (launch * 0xc2b2ae3d27d4eb4full);
  h ^= h >> 29;
  h *= 0xbf58476d1ce4e5b9ull;
  h ^= h >> 32;
  const uint32_t kind = (uint32_t)(h % 10);
  if (kind < 5) return (uint32_t)(h >> 8) % (quietBits + 1u);       // quiet, the threshold itself included
  if (kind < 6) return quietBits;                                   // exactly the threshold
  if (kind < 7) return 0x7fc00000u;                                 // a NaN
  return quietBits + 1u + (uint32_t)(h >> 8) % 1000u;               // loud
}

void walk(uint64_t seed, unsigned depth, int steps)
{
  const size_t V = 1000, maxListed = 200;
  Rig late(V, maxListed, depth);  // the object under test: results arrive when the walk says
  Rig sync(V, maxListed, depth);  // the same calls, every result taken in before each next_list
  Model model(V, maxListed, depth);
  Rng rng{seed};
  uint32_t quietBits = Q;
  uint64_t launch = 0;
  int lists = 0, busy = 0, ranges = 0, maxLate = 0, strictSupersets = 0;
  List cur, curSync;
  bool waiting = false;
  size_t lateness = 0;  // how many results the next_list calls leave out: 0 .. depth, changed now and then
  auto arrive = [&](size_t n) {
    late.fake.complete(n);
    model.arrive(n);
  };
  for (int step = 0; step < steps; ++step)
  {
    const uint32_t what = rng.below(100);
    if (rng.below(50) == 0) lateness = rng.below(3) == 0 ? depth : rng.below(depth + 1);
    if (what < 45)
    {
      // the next list: a must-set of 0 .. 24 voices, now and then an invalid one, now and then too little room
      List must;
      const uint32_t nMust = rng.below(4) == 0 ? 0 : rng.below(25);
      Set s;
      while (s.size() < nMust) s.insert(rng.below(V));
      must.assign(s.begin(), s.end());
      if (rng.below(40) == 0 && must.size() >= 2) must[1] = must[0];
      if (rng.below(40) == 0 && !must.empty()) must.back() = (uint32_t)V + rng.below(3);
      const size_t capacity = rng.below(25) == 0 ? rng.below(40) : 4096;
      if (late.tails.pending() > lateness) arrive(late.tails.pending() - lateness);
      List want;
      size_t wantN = 0;
      const int st = model.nextList(must, capacity, want, wantN);
      List got = late.next(must, st, capacity);
      CHECK(late.lastN == wantN || (st != MLGPU_OK && st != MLGPU_ERR_RANGE));
      CHECK(late.tails.pending() == model.outstanding());
      maxLate = (int)late.tails.pending() > maxLate ? (int)late.tails.pending() : maxLate;
      if (st == MLGPU_ERR_RANGE) ++ranges;
      if (st != MLGPU_OK) continue;
      CHECK(got == want);
      ++lists;
      cur = got;
      waiting = true;
      // (a) the synchronous object gets the same call with everything taken in: its list is within this one
      CHECK(sync.tails.wait() == MLGPU_OK);
      List small(4096);
      size_t nSmall = 0;
      CHECK(sync.tails.nextList(must.empty() ? nullptr : must.data(), must.size(), small.data(), small.size(), &nSmall) == MLGPU_OK);
      small.resize(nSmall);
      curSync = small;
      Set big(got.begin(), got.end());
      for (uint32_t v : small) CHECK(big.count(v) == 1);
      strictSupersets += got.size() > small.size() ? 1 : 0;
    }
    else if (what < 85)
    {
      // a note of 1 .. 3 DSPVectors
      List peaks(cur.size());
      const uint64_t j = ++launch;
      for (size_t i = 0; i < cur.size(); ++i) peaks[i] = peakOf(cur[i], j, quietBits);
      const size_t vectors = 1 + rng.below(3);
      static const uint32_t none = 0;
      const int want = model.note(vectors, peaks.empty() ? &none : peaks.data());
      const int st = late.note(vectors, peaks);
      CHECK(st == want);
      CHECK(late.tails.pending() == model.outstanding());
      busy += st == MLGPU_ERR_BUSY ? 1 : 0;
      // the same call for the synchronous object - a note that answered BUSY is no note
      if (st == MLGPU_OK && waiting)
      {
        List p2(curSync.size());
        for (size_t i = 0; i < curSync.size(); ++i) p2[i] = peakOf(curSync[i], j, quietBits);
        CHECK(sync.note(vectors, p2) == MLGPU_OK);
        sync.fake.complete(8);
      }
      if (st != MLGPU_ERR_INVALID) waiting = false;
    }
    else if (what < 88)
      arrive(1 + rng.below(depth));
    else if (what < 97)
    {
      // (c) wait, then list: the rule given every result
      const int waits = late.fake.waits;
      CHECK(late.tails.wait() == MLGPU_OK);
      model.wait();
      CHECK(late.tails.pending() == 0 && model.outstanding() == 0);
      CHECK(late.fake.flying.empty());
      CHECK(late.fake.waits >= waits);
    }
    else if (what < 99)
    {
      // (consequence (a) compares two runs under one hold, or one that was only raised: a lowered hold is a new start)
      const uint32_t hold = 1 + rng.below(6);
      if (hold < model.hold)
      {
        late.tails.clear();
        sync.tails.clear();
        model.clear();
        late.fake.complete(16);
        cur.clear();
        curSync.clear();
        waiting = false;
      }
      quietBits = rng.below(2) ? Q : 1000u + rng.below(1000);
      CHECK(late.tails.setThreshold(quietBits, hold) == MLGPU_OK && sync.tails.setThreshold(quietBits, hold) == MLGPU_OK);
      model.quietBits = quietBits;
      model.hold = hold;
    }
    else if (rng.below(4) == 0)
    {
      late.tails.clear();
      sync.tails.clear();
      model.clear();
      late.fake.complete(16);
      cur.clear();
      curSync.clear();
      waiting = false;
    }
  }
  printf("walk depth %u: %d steps, %d lists, %d BUSY, %d RANGE, up to %d results out, %d lists larger than the synchronous one, %d queries, %d waits\n", depth, steps,
         lists, busy, ranges, maxLate, strictSupersets, late.fake.queries, late.fake.waits);
  CHECK(lists > steps / 4 && busy > 0 && ranges > 0 && strictSupersets > 0);
  CHECK(maxLate == (int)depth);
  CHECK(late.fake.creates == (int)depth);
}
}  // namespace

int main()
{
  thresholdIsStrict();
  holdReachedExactly();
  resets();
  unNotedAndLate();
  busyAtDepth();
  clearForgets();
  refusalsLeaveTheStateIntact();
  setupRefusals();
  walk(1, 4, 24000);
  walk(2, 1, 4000);
  walk(3, 8, 6000);
  if (failures == 0) printf("All tests passed\n");
  return failures ? 1 : 0;
}
