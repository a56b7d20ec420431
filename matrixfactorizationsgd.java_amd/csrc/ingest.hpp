// ingest.hpp -- the seam between the host scheduler (schedule.cpp) and rating ingestion on the device (SURVEY.md 8f
// rank 1): degree histograms, COO -> (cell, sub-round, wave) bucket order and the per-cell step packer (pack.hip) on
// the GPU.  The scheduler writes no HIP call of its own: it sees the device through the one interface below and falls
// back to its own loops when there is none or a call fails; both produce identical arrays.  What the device packs
// comes back in DevBufs and stays in DevBufs.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

#include "devmem.hpp"
#include "records.hpp"

namespace mfsgd {

// ---- the per-cell step packer on the device (pack.hip) ---------------------------------------------
struct PackRequest {
    const float* r = nullptr;       // host: ratings of the loaded set
    const int64_t* orig = nullptr;  // host or null: caller-visible rating indices
    int32_t U = 0, I = 0;
    const int32_t* ubin = nullptr;  // host: fine bin of every P row / Q row (block = bin % B)
    const int32_t* ibin = nullptr;
    int B = 0, W = 0, G = 0, L = 0;
    float lr = 0.f, c = 0.f;
    bool solo_ok = false;
    int64_t max_cell_nnz = 0;       // from bptr
    // the most rows a chunk of the training kernel's LDS image can hold (0: not said).  A cell with more is cut whatever
    // it packs into, so the packing kernel need not provide for it: it reports such a cell as too large (status 2, row
    // counts valid) and keeps the smaller per-wave arrays -- and the better occupancy -- for everything else.
    int fit_rows = 0;
    // [r3] host, per cell, or null: where the cell's ratings start in the canonical order (it follows from the bucket
    // starts alone).  With it the COUNT pass also WRITES what it packs -- rows and entries into scratch arrays at
    // worst-case offsets, the order at its final place -- and emit() below only moves the cells that are kept to their
    // offsets: the packing runs once.  Without it (or when the scratch does not fit) emit() packs a second time.
    const int64_t* ord_off = nullptr;
};

// Where emit() writes the cells, from the COUNT pass: per cell (B*B entries each), and the totals.  A cell whose row_off
// is 0xFFFFFFFF is not the device's to write as a cell (it was cut: its chunks come as parts).
struct CellOffsets {
    const uint32_t* row_off = nullptr;
    const uint32_t* ent_off = nullptr;
    const int64_t* ord_off = nullptr;
    int64_t n_rows = 0, n_steps = 0;
    int64_t n_descs = 0;  // chunk descriptors of the schedule: B*B when no cell is cut
};

// [r3] Chunks on the device.  A chunk of a cell is a subset of its ratings (those inside a rectangle of user and item
// ids, schedule.cpp) packed as a complete little cell; to the packing kernel it IS a cell, given as a list: `sorted` =
// rating indices of the parts one after another, each in the cell's bucket order, `cptr` = n_parts * W*W + 1 sub-cell
// starts into that list.  For emit(), also where each part goes.
struct PartsToEmit {
    int64_t n_parts = 0, n_sorted = 0;
    const uint32_t* sorted = nullptr;
    const int64_t* cptr = nullptr;
    const uint32_t *row_off = nullptr, *ent_off = nullptr;  // per part
    const int64_t* ord_off = nullptr;
    const int64_t* desc = nullptr;  // the chunk descriptor of every part (final sub-cell table)
};

// What a successful emit() leaves on the device, owned: the schedule holds it until the first compute call moves rows,
// entries and subs into the partition's own arrays (the order stays: only mfsgd_get_order reads it).
struct DevicePacked {
    DevArray<uint32_t> rows;  // n_rows (+4 padding words)
    DevArray<Entry> entries;  // n_entries
    DevArray<int64_t> order;  // n
    // [r3] the sub-cell tables of all chunk descriptors (n_subs SubDesc records, the two padding records included): the
    // device wrote them and the training kernel reads them, so they need not come to the host and go back
    DevArray<SubDesc> subs;
    int64_t n_subs = 0;
};

// Every call works on the rating set that was loaded and returns 0 on success, -1 when a HIP call failed (or nothing
// fitting is loaded): the host loops take over.
struct DeviceIngest {
    virtual ~DeviceIngest() = default;
    // The rating set of the calls that follow: n triples in host arrays that stay valid until drop() or the next
    // load().  Whatever was derived from an earlier set goes.  The copy to the device is made by the first call that
    // needs it.
    virtual void load(const int32_t* u, const int32_t* i, int64_t n) = 0;
    virtual void drop() = 0;
    virtual int64_t loaded() const = 0;  // n of the loaded set, -1: none
    // degu[U], degi[I]: number of ratings per row.
    virtual int degrees(int32_t U, int32_t I, int64_t* degu, int64_t* degi) = 0;
    // Stable sort of the rating indices by bucket key
    //   key = (((ub * B + it) * W + s) * W + us),  ub = ubin[u] % B, us = ubin[u] / B, it = ibin[i] % B,
    //   is = ibin[i] / B, s = (is - us + W) % W; an item with a tile of its own (ibin[i] < giants: schedule.cpp,
    //   lpt_assign) takes us = 0 for all its ratings -- its tile holds nothing else, so its cells are ONE sub-cell
    // bptr[nb + 1] = first position of every bucket, sorted[n] = rating indices in key order (ties in input order).
    virtual int bucket(const int32_t* ubin, const int32_t* ibin, int32_t U, int32_t I, int B, int W, int giants, int64_t* bptr,
                       int64_t* sorted) = 0;
    // the same, but the sorted indices stay on the device for the packer (only bptr comes back)
    virtual int bucket_dev(const int32_t* ubin, const int32_t* ibin, int32_t U, int32_t I, int B, int W, int giants,
                           int64_t* bptr) = 0;
    // the sorted indices after bucket_dev (the 32-bit indices the device holds), for the host packer (fallback)
    virtual int fetch_sorted32(uint32_t* sorted) = 0;
    // [r3] ... and only `n_ranges` pieces of them -- positions [lo[x], lo[x] + len[x]) of the bucket order, concatenated
    // into `out` (sum of len entries): the cells whose chunks the host has to decide (a gather on the device, ONE copy)
    virtual int fetch_sorted_ranges(int64_t n_ranges, const int64_t* lo, const int64_t* len, uint32_t* out) = 0;
    // COUNT pass: 0 = done (info: B*B; the cells' sub-cell tables stay on the device), 1 = this rating set is outside
    // what the kernel handles (nothing produced), -1 = a HIP call failed
    virtual int pack_count(const PackRequest& req, std::vector<PackCellInfo>& info) = 0;
    // [r3] COUNT over a list of parts (any number of times, between pack_count and emit): info[n_parts]; the offsets
    // of `parts` are not read.
    virtual int pack_count_parts(const PartsToEmit& parts, PackCellInfo* info) = 0;
    // EMIT pass: the whole cells at `cells`' offsets and, when there are `parts` (null: none), the final list of the
    // chunks of the cells that were cut, each at its offsets, into ONE set of arrays.  out.subs = the final sub-cell
    // table of all n_descs chunk descriptors: the cells' tables as counted, the parts' tables at their descriptors,
    // zeros elsewhere and in the two padding records.
    virtual int emit(const CellOffsets& cells, const PartsToEmit* parts, DevicePacked& out) = 0;
};

// Implemented in ingest.hip.  `device` must already be usable (ratings.cpp checks).
std::unique_ptr<DeviceIngest> make_device_ingest(int device);

}  // namespace mfsgd
