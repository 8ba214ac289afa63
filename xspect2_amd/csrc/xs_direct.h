// xs_direct.h — pieces shared by the direct probes (xs_probe_fast/vslice/wide/
// slots/general.hip, xs_probe_bloom.hip), the builders (xs_kernels.hip) and
// bloom_count_kernel (xs_probe_bloompart.hip).  Every one of them decodes a
// unit with unit_at.  The queue walk, the COBS hashes and the hit-row store are
// used by the kernels whose registers, scratch and speed they leave as they
// were: walk_units by general, rbloom and the builders; cobs_hashes by fast,
// general and build_cobs_kernel; store_hit by vslice, general, rbloom and
// bloom_count_kernel.  The other kernels keep their own copy of a piece, each
// for a reason recorded per kernel in profiles/direct_shared_refactor.txt; a
// change to a piece is made here and in those copies.  The gathers, the
// counting, the LDS layouts and the partials stay with each family.
#pragma once
#include "xs_device.h"

namespace xs {

// ------------------------------------------------------------------ units
// One unit: k-mers t0 .. t0 + cnt - 1 (cnt <= kSegKmers) of the nk sampled
// k-mers of read r, whose len bytes start at o0.
struct Unit {
    uint32_t r;
    uint64_t o0, len, nk, t0;
    uint32_t cnt;
    // the read's only unit: its hit row is stored, not added to (store_hit)
    __device__ __forceinline__ bool whole() const { return nk <= kSegKmers; }
};

__device__ __forceinline__ Unit unit_at(const ReadView& rv, uint64_t u, uint32_t k, uint32_t step) {
    Unit n;
    n.r = rv.unit_read[u];
    const uint64_t seg = u - rv.unit_ofs[n.r];
    n.o0 = rv.offs[n.r];
    n.len = rv.offs[n.r + 1] - n.o0;
    n.nk = num_kmers(n.len, k, step);
    n.t0 = seg * kSegKmers;
    n.cnt = (uint32_t)min((uint64_t)kSegKmers, n.nk - n.t0);
    return n;
}

// One wavefront per unit: the wave takes rv.grab units at a time from the
// queue until it is empty and runs body(unit) on each.
template <class Body>
__device__ __forceinline__ void walk_units(const ReadView& rv, int lane, uint32_t k, uint32_t step, Body body) {
    const uint64_t U = rv.queue[0];
    for (;;) {
        const uint64_t base = grab_units(rv.queue, lane, rv.grab);
        if (base >= U) break;
        const uint64_t uend = min(base + rv.grab, U);
        for (uint64_t u = base; u < uend; ++u) body(unit_at(rv, u, k, step));
    }
}

// ------------------------------------------------------------------ hashes
// put(j, XXH64 with seed j of the canonical k-mer at read position p of the
// unit's read) for j < h <= NH.  The caller takes each hash as it comes (fast
// keeps 32-bit row offsets, not the hashes); what it holds for j >= h stays as
// it set it.
template <int KT, int NH, class Put>
__device__ __forceinline__ void cobs_hashes(const ReadView& rv, const Unit& n, uint64_t p, uint32_t k, uint32_t h,
                                            Put put) {
    Kmer c;
    kmer_at<KT, kKmerCobs>(rv, n.o0, n.len, p, k, c);
    Xxh64Pre pre;
    xxh64_pre<KT>(c, k, pre);
#pragma unroll
    for (int j = 0; j < NH; ++j)
        if ((uint32_t)j < h) put(j, xxh64_seed<KT>(c, pre, k, (uint64_t)j));
}

// ------------------------------------------------------------------ hit rows
// Whole unit stores, split unit adds: the row of a read with
// one unit is written without having been zeroed; the rows of the others are
// zeroed by scatter_units_kernel and summed here.  The caller asks first
// whether there is a hit matrix, before it forms the index.
__device__ __forceinline__ void store_hit(uint32_t* hits, uint64_t i, uint32_t v, bool whole) {
    if (whole) hits[i] = v;
    else if (v) atomicAdd(&hits[i], v);
}

}  // namespace xs
