// param_updates.hpp — the HOST half of sparse per-voice table updates (mlgpu_graph_apply_updates / mlgpu_bank_apply_updates): a list
// of mlgpu_update records is validated against a description of the object's tables, MLGPU_UPDATE_CLEAR is expanded into one record
// per cleared state word, overlapping records are found and the list is cut into batches none of which writes a word twice, and the
// result is packed as 16-byte device records straight into the caller's (pinned) upload buffer. MLGPU_UPDATE_CLEAR_RINGS adds the
// zero fills of a voice range's delay-ring words, as strided spans of the ring memory worked out from the ring layout (RingRec, two
// 16-byte slots each, behind the table records). Plain C++ that never touches a device: built and tested without any HIP header;
// updates.hip is the caller.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/mlgpu.h"

namespace mlupd
{
enum Table : uint32_t { TABLE_PARAMS = 0, TABLE_COEFFS = 1, TABLE_STATE = 2, TABLE_INPUT_CONST = 3, kTables = 4 };

// What apply_updates_kernel reads, one dwordx4 load per record: `bits` goes to words [first, first + count) of row `row` of `table`
struct DevRec
{
  uint32_t tableRow;  // table << 30 | row
  uint32_t first, count, bits;
};
constexpr uint32_t kRowBits = 30, kRowMask = (1u << kRowBits) - 1u;
inline DevRec makeRec(uint32_t table, uint32_t row, uint32_t first, uint32_t count, uint32_t bits) { return DevRec{(table << kRowBits) | row, first, count, bits}; }

// What clear_rings_kernel reads, two dwordx4 loads per record: zeros to `rows` spans of `span` contiguous words, `stride` words
// apart, the first at word `offset` of the graph's ring memory. One record per (node, segment of the voice range): in ring layout
// ROWS ([ring position][voice]) the whole range - span = voices, stride = V, rows = the node's ring words per voice; in the
// windowed layouts ([256-voice block][granule of the ring][lane][G words]) the part of the range inside one 256-voice block - span
// = voices * G, stride = 256 * G, rows = ring words per voice / G. Zero fills commute and touch no table: ring records take no
// part in overlap detection or batch cutting.
struct RingRec
{
  uint64_t offset;
  uint32_t span, stride, rows;
  uint32_t pad[3];
};
static_assert(sizeof(RingRec) == 2 * sizeof(DevRec), "a ring record is two slots of the staging buffer");

// The rows one node (graph) / processor (bank) owns
struct NodeDesc
{
  enum Kind { OTHER = 0, PARAM, PROC, FEEDBACK };
  int kind{OTHER};
  int paramRow{0};              // PARAM: its row of the params table
  int cOff{0}, nc{0};           // PROC: rows [cOff, cOff + nc) of the coefficient table
  int sOff{0}, ns{0};           // PROC / FEEDBACK: rows [sOff, sOff + ns) of the state table
  bool rings{false};            // owns delay rings: MLGPU_UPDATE_CLEAR is refused, MLGPU_UPDATE_CLEAR_RINGS zeroes them
  uint64_t memOff{0};           // ... which start at word memOff * memVoices of the ring memory,
  uint64_t ringWords{0};        // ringLen * rings words per voice (a multiple of the layout's granule)
  std::vector<uint32_t> clearWords;  // [ns] T::clear()'s value of each state word ...
  std::vector<uint8_t> clearMask;    // [ns] ... and whether clear() resets it at all
};
struct TableDesc
{
  bool bank{false};  // bank: node = processor index, no params, an input-const table; graph: the other way round
  size_t V{0};
  // a graph's ring memory: the words a voice owns in one piece (1: layout ROWS, 8: WINDOWS and SECTORS, 16: TRANSPOSED), the voices
  // it is laid out for (V, or whole 256-voice blocks), and whether the spare lanes of a last wavefront that is not full run the last
  // voice again on ring memory of their own (layout TRANSPOSED with V % 64 != 0): a clear of voice V - 1 then clears theirs too
  uint32_t ringGranule{1};
  size_t memVoices{0};
  bool spareLanes{false};
  std::vector<NodeDesc> nodes;
};

class UpdatePlanner
{
 public:
  // room for lists of up to maxDeviceRecords device records: no call below allocates while a list stays within it
  void reserve(size_t maxDeviceRecords);

  // MLGPU_OK, or the status of the first bad record with error() naming its position. Nothing is written anywhere.
  int validate(const TableDesc& d, const mlgpu_update* recs, size_t n);
  // of the list validated last (0 after a refusal): 16-byte slots in all = tableRecords() + 2 * ringRecords()
  size_t deviceRecords() const { return nDev; }
  size_t tableRecords() const { return nTable; }
  size_t ringRecords() const { return (nDev - nTable) / 2; }
  const char* error() const { return err; }

  // The list validated last, expanded and packed in list order into dst[deviceRecords()] - the table records first, the ring
  // records (RingRec) from dst + tableRecords() on - and the table records cut into batches: batch b is
  // dst[batchEnd(b - 1), batchEnd(b)), no two records of a batch share a word, and batches applied in order leave what the
  // records applied one at a time in list order leave.
  void pack(const TableDesc& d, const mlgpu_update* recs, size_t n, DevRec* dst);
  size_t batches() const { return ends.size(); }
  size_t batchEnd(size_t b) const { return ends[b]; }

 private:
  bool disjoint(const DevRec* r, size_t s, size_t e);
  size_t nDev{0}, nTable{0};
  std::vector<uint32_t> order;  // scratch: record indices sorted by (table, row, first)
  std::vector<size_t> ends;
  char err[256]{0};
};
}  // namespace mlupd
