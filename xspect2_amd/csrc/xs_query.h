// xs_query.h — what xs_query.cpp shares with xs_mlst.cpp: the probe dispatcher, the chunked host
// pipeline and the host <-> device copy helpers.  Host only, not part of the public ABI.
#pragma once
#include "xs_host.h"

namespace xs {

struct Inputs {
    const uint8_t* seqs;
    uint64_t seq_bytes;      // readable bytes from seqs (window loads stop there)
    const uint64_t* offs;
    uint64_t n;
    uint64_t read_bytes = 0;  // bytes of these n reads (plans and bounds); 0: seq_bytes
    uint64_t plan_bytes() const { return read_bytes ? read_bytes : seq_bytes; }
};

// Enqueue one query on device buffers.  d_totals: cols() + 1 entries.
int run_query(xs_bank* b, const Inputs& in, uint32_t step, uint32_t* d_hits, uint64_t* d_nk, uint64_t* d_totals,
              hipStream_t s);

// Reads already in HBM (a device-mode reader's batch): query_host then only
// chunks the probe and the hit-row D2H.
struct DevReads {
    const uint8_t* seqs;
    uint64_t seq_bytes;
    const uint64_t* offs;  // n+1, offs[0] = 0
};

// One call of query_host: where the n reads are, and what the caller wants back.
struct HostQuery {
    const char* seqs;         // reads on the host: their bytes and n + 1 offsets as the caller gave them ...
    const uint64_t* offsets;
    const DevReads* dev;      // ... or reads on the device (seqs and offsets null); chunks are then cut by read count
    uint64_t n;
    uint32_t step;
    uint32_t* d_hits = nullptr;    // n x cols uint32 rows on the device
    // the rows back on the host (needs d_hits) as hit_bytes-wide counts, crossing PCIe wire_bytes wide (0: hit_bytes;
    // narrower: narrowed on the device into b->narrow, widened on the host; the caller checked that they fit)
    void* hits_host = nullptr;
    int hit_bytes = 4, wire_bytes = 0;
    uint64_t* d_nk = nullptr;      // per-read k-mer counts on the device
    uint64_t* tot_host = nullptr;  // cols + 1 entries on the host: per-doc sums, then the k-mer total
};
int query_host(xs_bank* b, const HostQuery& q);

// However a call ends, nothing enqueued for it on s may still read the caller's memory once it has returned.
struct DrainStream {
    hipStream_t s = nullptr;
    ~DrainStream() {
        if (s) (void)hipStreamSynchronize(s);
    }
};

// dst[r] = offsets[r] - offsets[0] for the n + 1 offsets of n reads, in one pass on several
// threads; false when a pair of offsets decreases
bool rebase_offsets(const uint64_t* offsets, uint64_t n, uint64_t* dst);
int bad_offsets();

// Host reads into b's device buffers on stream s (offsets rebased to 0, kept in b->offs_h for the
// call): pageable bytes go through the pinned H2D ring, the copy of slot i behind the host's fill of
// slot i+1.  The caller synchronises s before the source memory may change.
int upload_reads(xs_bank* b, const char* seqs, const uint64_t* offsets, uint64_t n, hipStream_t s, Inputs* in);

// Several device regions -> host memory, ordered after the work already on `st`; returns once
// they are there.  A part of ring_min bytes or more bound for pageable memory crosses in 32 MiB
// pieces through the two pinned slots of b->stage, the DMA of one piece behind the host threads'
// copy of the one before (a plain pageable D2H runs at about 9 GB/s on the box, a pinned one at
// PCIe rate); the others are plain copies.
struct D2hPart {
    void* host;
    const void* dev;
    size_t bytes;
};
int d2h_parts(xs_bank* b, const D2hPart* parts, int n_parts, size_t ring_min, hipStream_t st);

}  // namespace xs
