// xs_mlst_ranks.hip — per record and locus, the N best alleles of an MLST locus on the device.
//
// The reference keeps the first `limit_number` (5) items of each locus' result under "All results"
// (probabilistic_filter_mlst_model.py:258-259, 278-282): for a record probed whole the COBS order of
// its hit row (count descending, ties by doc index), for a chunked record the stable sort by -sum of
// the alleles some chunk kept (:248-256).  Rank 0 is the call xs_mlst_top.hip and
// mlst_owner_top_kernel make; the ranks behind it say between which alleles a call is close.
//
// Both kernels are one wavefront per row, the row read once with the head / 16-byte body / tail
// peeling of the top-1 kernels.  Each lane keeps the CAP best entries it met, ordered, in registers:
// CAP is a template parameter and every loop over the entries is unrolled, so no entry is indexed
// at run time.  An entry that does not beat the lane's CAP-th best is rejected by one compare.  The
// wave then takes N rounds of a maximum across the lanes' heads; the lane that held it drops its
// head.  One lane may hold several of the N ranks or (D < 64) none.  No LDS, no scratch.
#include "xs_device.h"

namespace xs {

namespace {

// The CAP best entries one lane met, best first.  E: a value type with beats(other) (a strict
// order in which every real entry beats the empty one, E{}) and pick(c, a, b) = c ? a : b member
// by member, arguments by value (a select between two references is one between addresses, and
// sends the array to scratch).
template <class E, int CAP>
struct LaneBestN {
    E e[CAP];
    __device__ __forceinline__ void take(E x) {
        if (!x.beats(e[CAP - 1])) return;
#pragma unroll
        for (int i = CAP - 1; i >= 1; --i) e[i] = E::pick(x.beats(e[i - 1]), e[i - 1], E::pick(x.beats(e[i]), x, e[i]));
        e[0] = E::pick(x.beats(e[0]), x, e[0]);
    }
    __device__ __forceinline__ void pop() {
#pragma unroll
        for (int i = 0; i + 1 < CAP; ++i) e[i] = e[i + 1];
        e[CAP - 1] = E{};
    }
};

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, shfl_xor_u64(v, o));
    return v;
}
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, shfl_xor_u64(v, o));
    return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
    return v;
}

// A count and its doc as one unsigned key, count << 32 | ~doc: the larger key is the higher count,
// then the lower doc (COBS order).  A doc is below 2^32 - 1, so a real key is never 0, the empty one.
struct RowEntry {
    uint64_t k = 0;
    __device__ __forceinline__ bool beats(const RowEntry& o) const { return k > o.k; }
    static __device__ __forceinline__ RowEntry pick(bool c, RowEntry a, RowEntry b) {
        return RowEntry{c ? a.k : b.k};
    }
};

// A chunked record's allele: sum descending, then key ascending (first passing chunk, then the
// higher count there), then doc ascending.  s == 0: empty (only alleles with a sum > 0 take part).
struct OwnerEntry {
    uint64_t s = 0, key = ~0ull;
    uint32_t doc = kMlstNone;
    __device__ __forceinline__ bool beats(const OwnerEntry& o) const {
        return s > o.s || (s == o.s && (key < o.key || (key == o.key && doc < o.doc)));
    }
    static __device__ __forceinline__ OwnerEntry pick(bool c, OwnerEntry a, OwnerEntry b) {
        return OwnerEntry{c ? a.s : b.s, c ? a.key : b.key, c ? a.doc : b.doc};
    }
};

}  // namespace

// One wave per hit row of D counts.  Rank j of row r goes to rank_*[r * rank_stride + j]; top,
// top_score and n_tied (each may be null) are xs_mlst_top.hip's, from the same pass.
template <int CAP>
__global__ void __launch_bounds__(256) mlst_ranks_kernel(const uint32_t* __restrict__ hits, uint64_t n, uint64_t D,
                                                         uint32_t n_ranks, uint32_t* __restrict__ top,
                                                         uint32_t* __restrict__ top_score,
                                                         uint32_t* __restrict__ n_tied, uint64_t top_stride,
                                                         uint32_t* __restrict__ rank_allele,
                                                         uint32_t* __restrict__ rank_score, uint64_t rank_stride) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t r = wave; r < n; r += waves) {
        const uint32_t* row = hits + r * D;
        const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(row) >> 2) & 3u;
        const uint32_t head = (uint32_t)min((uint64_t)((4u - mis) & 3u), D);
        const uint32_t nvec = (uint32_t)((D - head) >> 2);
        const uint32_t tail0 = head + 4u * nvec;
        LaneBestN<RowEntry, CAP> best;
        uint32_t m = 0, cnt = 0;  // the lane's maximum and the docs holding it; cnt == 0: nothing seen yet
        auto take = [&](uint32_t v, uint32_t d) {
            if (cnt == 0 || v > m) {
                m = v;
                cnt = 1;
            } else if (v == m) {
                ++cnt;
            }
            best.take(RowEntry{((uint64_t)v << 32) | (uint32_t)~d});
        };
        if (lane < head) take(row[lane], lane);
        const uint4* body = reinterpret_cast<const uint4*>(row + head);
        for (uint32_t i = lane; i < nvec; i += 64) {
            const uint4 v = body[i];
            const uint32_t d = head + 4u * i;
            take(v.x, d);
            take(v.y, d + 1);
            take(v.z, d + 2);
            take(v.w, d + 3);
        }
        if (tail0 + lane < D) take(row[tail0 + lane], tail0 + lane);
        // N rounds: the best head of the wave is rank j; lane j keeps it, the lane that held it drops it
        uint64_t mine = 0, first = 0;
        for (uint32_t j = 0; j < n_ranks; ++j) {
            const uint64_t w = wave_max_u64(best.e[0].k);
            if (w != 0 && best.e[0].k == w) best.pop();
            if (lane == j) mine = w;
            if (j == 0) first = w;
        }
        if (lane < n_ranks) {
            const uint64_t o = r * rank_stride + lane;
            rank_allele[o] = mine ? ~(uint32_t)mine : kMlstNone;
            rank_score[o] = (uint32_t)(mine >> 32);
        }
        if (top || top_score || n_tied) {  // D >= 1: rank 0 exists
            const uint32_t wm = (uint32_t)(first >> 32);
            uint32_t c = (cnt && m == wm) ? cnt : 0;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o, 64);
            if (lane == 0) {
                const uint64_t o = r * top_stride;
                if (top) top[o] = ~(uint32_t)first;
                if (top_score) top_score[o] = wm;
                if (n_tied) n_tied[o] = c;
            }
        }
    }
}

// One wave per owner over its D (sum, key) accumulators of mlst_chunk_acc_kernel, read as
// mlst_owner_top_kernel reads them.  Rank j of owner o goes to rank_*[row * rank_stride + j],
// row = rec ? rec[o * rec_stride] : o.
template <int CAP>
__global__ void __launch_bounds__(256) mlst_owner_ranks_kernel(const unsigned long long* __restrict__ sum,
                                                               const unsigned long long* __restrict__ key,
                                                               uint64_t n_owners, uint64_t D,
                                                               const uint64_t* __restrict__ rec, uint32_t rec_stride,
                                                               uint32_t n_ranks, uint32_t* __restrict__ rank_allele,
                                                               uint32_t* __restrict__ rank_score,
                                                               uint64_t rank_stride) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t o = wave; o < n_owners; o += waves) {
        const unsigned long long* srow = sum + o * D;
        const unsigned long long* krow = key + o * D;
        const uint32_t head = (uint32_t)min((uint64_t)((reinterpret_cast<uintptr_t>(srow) >> 3) & 1u), D);
        const bool kvec = ((reinterpret_cast<uintptr_t>(krow + head)) & 15u) == 0;
        const uint32_t nvec = (uint32_t)((D - head) >> 1);
        const uint32_t tail0 = head + 2u * nvec;
        LaneBestN<OwnerEntry, CAP> best;
        auto take = [&](uint64_t v, uint64_t kk, uint32_t d) {
            if (v != 0) best.take(OwnerEntry{v, kk, d});
        };
        if (lane < head) take(srow[lane], krow[lane], lane);
        const ulonglong2* sbody = reinterpret_cast<const ulonglong2*>(srow + head);
        for (uint32_t i = lane; i < nvec; i += 64) {
            const ulonglong2 sv = sbody[i];
            const uint32_t d = head + 2u * i;
            ulonglong2 kv;
            if (kvec) {
                kv = reinterpret_cast<const ulonglong2*>(krow + head)[i];
            } else {
                kv.x = krow[d];
                kv.y = krow[d + 1];
            }
            take(sv.x, kv.x, d);
            take(sv.y, kv.y, d + 1);
        }
        if (tail0 + lane < D) take(srow[tail0 + lane], krow[tail0 + lane], tail0 + lane);
        // N rounds of the lexicographic maximum over the lanes' heads: the largest sum, over its lanes
        // the lowest key, over those the lowest doc; that doc's lane drops its head
        uint32_t my_doc = kMlstNone, my_score = 0;
        for (uint32_t j = 0; j < n_ranks; ++j) {
            const OwnerEntry h = best.e[0];
            const uint64_t ws = wave_max_u64(h.s);
            const bool in = ws != 0 && h.s == ws;
            const uint64_t wk = wave_min_u64(in ? h.key : ~0ull);
            const uint32_t a = wave_min_u32((in && h.key == wk) ? h.doc : kMlstNone);
            if (in && h.key == wk && h.doc == a) best.pop();
            if (lane == j) {
                my_doc = ws ? a : kMlstNone;
                my_score = (uint32_t)ws;
            }
        }
        if (lane < n_ranks) {
            const uint64_t w = (rec ? rec[o * rec_stride] : o) * rank_stride + lane;
            rank_allele[w] = my_doc;
            rank_score[w] = my_score;
        }
    }
}

// Compiled capacities: 2, 5 (the reference's limit_number) and 8 (kMlstMaxRanks); a call takes the
// smallest that holds its n_ranks.
hipError_t launch_mlst_ranks(const uint32_t* hits, uint64_t n, uint64_t D, uint32_t n_ranks, uint32_t* top,
                             uint32_t* top_score, uint32_t* n_tied, uint64_t top_stride, uint32_t* rank_allele,
                             uint32_t* rank_score, uint64_t rank_stride, hipStream_t s) {
    if (n == 0 || D == 0) return hipSuccess;
    if (n_ranks == 0 || n_ranks > kMlstMaxRanks) return hipErrorInvalidValue;
    const int grid = grid_for(n, 4, 16384);
    if (n_ranks <= 2)
        mlst_ranks_kernel<2><<<grid, 256, 0, s>>>(hits, n, D, n_ranks, top, top_score, n_tied, top_stride,
                                                  rank_allele, rank_score, rank_stride);
    else if (n_ranks <= 5)
        mlst_ranks_kernel<5><<<grid, 256, 0, s>>>(hits, n, D, n_ranks, top, top_score, n_tied, top_stride,
                                                  rank_allele, rank_score, rank_stride);
    else
        mlst_ranks_kernel<8><<<grid, 256, 0, s>>>(hits, n, D, n_ranks, top, top_score, n_tied, top_stride,
                                                  rank_allele, rank_score, rank_stride);
    return hipGetLastError();
}

hipError_t launch_mlst_owner_ranks(const unsigned long long* sum, const unsigned long long* key, uint64_t n_owners,
                                   uint64_t D, const uint64_t* rec, uint32_t rec_stride, uint32_t n_ranks,
                                   uint32_t* rank_allele, uint32_t* rank_score, uint64_t rank_stride, hipStream_t s) {
    if (n_owners == 0 || D == 0) return hipSuccess;
    if (n_ranks == 0 || n_ranks > kMlstMaxRanks) return hipErrorInvalidValue;
    const int grid = grid_for(n_owners, 4, 16384);
    if (n_ranks <= 2)
        mlst_owner_ranks_kernel<2><<<grid, 256, 0, s>>>(sum, key, n_owners, D, rec, rec_stride, n_ranks, rank_allele,
                                                        rank_score, rank_stride);
    else if (n_ranks <= 5)
        mlst_owner_ranks_kernel<5><<<grid, 256, 0, s>>>(sum, key, n_owners, D, rec, rec_stride, n_ranks, rank_allele,
                                                        rank_score, rank_stride);
    else
        mlst_owner_ranks_kernel<8><<<grid, 256, 0, s>>>(sum, key, n_owners, D, rec, rec_stride, n_ranks, rank_allele,
                                                        rank_score, rank_stride);
    return hipGetLastError();
}

}  // namespace xs
