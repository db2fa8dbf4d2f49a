// voice_records.hpp — the HOST half of voice records (mlgpu_graph_export_voices / _import_voices and the bank's): the layout of one
// voice's whole state as a record of W 32-bit words, the signature that says which objects exchange records, and the work list of a
// call - segments (what a record is made of) and entries (which voice slot goes with which record) - packed for the two kernels of
// voice_records.hip. Worked out from the mlupd::TableDesc the sparse updates already keep. Plain C++ that never touches a device:
// built and tested without any HIP header.
//
// A record, in words (an exact image: write indices and every other state word go as they are):
//   [0, nParams)                     the voice's word of params row 0, 1, ...
//   [.., + nCoeffs)                  of coefficient row 0, 1, ...
//   [.., + nState)                   of state row 0, 1, ... (a feedback node's stored vector is 64 of them)
//   [.., + 1)                        a bank's input-const word
//   (zeros up to a multiple of 4)
//   then node by node, in node order, the node's ringWords ring words in ascending address order of the voice's own ring memory:
//   record word r of the node is
//     ring layout ROWS (granule 1):   word memOff * V + r * V + v                                  of the ring memory
//     the windowed layouts (G words): word memOff * memVoices + (v >> 8) * ringWords * 256 + (v & 255) * G + (r / G) * 256 * G + r % G
//   W is the total, a multiple of 4: records in a buffer [n][W] are 16-byte aligned, and so is every node's ring part.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "param_updates.hpp"

namespace mlrec
{
constexpr uint32_t kFormatVersion = 1;

// What the signature covers of a node besides the rows the TableDesc has (nc, ns): the node's type and kind as the owner numbers them
// (a graph: mlgraph::NodeType and the processor kind or op; a bank: 3 and the processor kind), the ring length and the ring count
struct NodeSig
{
  int32_t type{0}, kind{0};
  uint32_t ringLen{0}, rings{0};
};

// One piece of a record, as the kernels read it (two dwordx4 loads): `rows` words per voice that lie `recOff` words into the record.
// where < kRing: rows of V words of table `where` (mlupd::Table), the voice's word of row r at r * V + v.
// where == kRing: a node's ring words, at `base` (memOff * V, or memOff * memVoices) of the ring memory, by the layout's address map.
constexpr uint32_t kRing = mlupd::kTables;
struct Segment
{
  uint64_t base;
  uint32_t rows, recOff, where;
  uint32_t pad[3];
};
static_assert(sizeof(Segment) == 32, "a segment is two 16-byte slots of the staging buffer");

// Which voice slot goes with which record of the caller's buffer. A slot >= V is a spare lane's ring memory (ring layout TRANSPOSED,
// V % 64 != 0: the lanes behind the last voice run it again on rings of their own): its rings take the record, tables have no such row.
struct Entry
{
  uint32_t slot, record;
};

class RecordPlan
{
 public:
  // The layout and the signature of an object: `sigs` one per node of d; ringLayout the layout the plan resolved to, as the API numbers
  // it (0, 1, 2, 4; a bank: 0); revision mlgpu_behaviour_revision(). false (error() says why): the object has no record layout.
  bool describe(const mlupd::TableDesc& d, const std::vector<NodeSig>& sigs, int ringLayout, int revision);
  bool described() const { return W != 0; }
  size_t words() const { return W; }
  uint64_t signature() const { return sig; }
  size_t tableWords() const { return nTableWords; }          // params + coefficients + state (+ input const)
  const std::vector<Segment>& segments() const { return segs; }
  uint32_t granule() const { return G; }
  size_t voices() const { return V; }

  // (no call below allocates: describe() made the one scratch they need)
  // MLGPU_OK, or the refusal's status with error() naming the position. Export: any voices below V. Import: distinct ones.
  int validate(const uint32_t* voices, size_t n, bool import);
  // of the call validated last: entries (import of voice V - 1 adds the spare lanes), and the 32-bit words of the upload
  size_t entries() const { return nEntries; }
  size_t uploadWords() const { return uploadWordsFor(nEntries); }
  size_t uploadWordsFor(size_t nE) const { return segs.size() * (sizeof(Segment) / 4) + 2 * nE; }
  static size_t maxEntries(size_t nVoices) { return nVoices + 63; }
  // the segments, then the entries, into dst[uploadWords()]
  void pack(const uint32_t* voices, size_t n, bool import, uint32_t* dst) const;
  const char* error() const { return err; }

 private:
  size_t V{0}, memVoices{0}, W{0}, nTableWords{0}, nEntries{0};
  uint32_t G{1};
  bool spareLanes{false};
  uint64_t sig{0};
  std::vector<Segment> segs;
  std::vector<uint64_t> seen;  // a bit per voice: import's distinctness check (all zero between calls)
  char err[256]{0};
};
}  // namespace mlrec
