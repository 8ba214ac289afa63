// xs_filter.hip — gfx950 kernels of read filtering: the keep decision over a device hit matrix and the
// order-preserving compaction of the kept reads (their index and output offsets).
//
// Reference semantics restated: ModelResult.get_filter_mask (src/xspect/models/result.py:92-123) keeps a
// read when round(h / n, 2) >= threshold, or with threshold -1 when the label's rounded score is the
// read's largest.  round(x, 2) is monotone in the double x, so the 101 cuts of xs_filter_cuts (cut[c] =
// the smallest double that rounds to c/100 or more) turn the decision into comparisons: centi(x) = the
// number of cuts <= x, minus one.  x = (double)h / (double)n is an IEEE double division (this file is
// built without fast-math; tests/test_filter_cuts.py checks the flags).
#include "xs_device.h"

namespace xs {

namespace {

// ------------------------------------------------------------------ keep
// Threshold mode: centi(x) >= c_min <=> x >= cut[c_min], one comparison per read and only the label's
// column of the row.  One thread per read (D = 1, the genus filter: three coalesced streams).
__global__ void __launch_bounds__(256) filter_keep_threshold_kernel(const uint32_t* __restrict__ hits,
                                                                    const uint64_t* __restrict__ nk, uint64_t n,
                                                                    uint64_t D, uint64_t label, double cut_min,
                                                                    uint8_t* __restrict__ keep,
                                                                    uint32_t* __restrict__ label_hits) {
    for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t h = hits[r * D + label];
        const uint64_t k = nk[r];
        keep[r] = k != 0 && (double)h / (double)k >= cut_min;
        if (label_hits) label_hits[r] = h;
    }
}

// Max mode, D > kKeepRowDocs: one wavefront per read, lanes stride over the unmasked docs for the row's maximum; the read
// is kept when the label's centi-value equals the maximum's.
__global__ void __launch_bounds__(256) filter_keep_max_kernel(const uint32_t* __restrict__ hits,
                                                              const uint64_t* __restrict__ nk, uint64_t n, uint64_t D,
                                                              uint64_t label, const uint8_t* __restrict__ mask,
                                                              FilterCuts cuts, uint8_t* __restrict__ keep,
                                                              uint32_t* __restrict__ label_hits) {
    __shared__ double s_cut[kFilterCuts];
    for (int i = threadIdx.x; i < kFilterCuts; i += blockDim.x) s_cut[i] = cuts.c[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t r = wave; r < n; r += waves) {
        const uint32_t* row = hits + r * D;
        uint32_t m = 0;
        for (uint64_t d = (uint64_t)lane; d < D; d += 64)
            if (!mask || mask[d]) m = max(m, row[d]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
        if (lane == 0) {
            const uint32_t h = row[label];
            const uint64_t k = nk[r];
            keep[r] = k != 0 && filter_centi((double)h / (double)k, s_cut) == filter_centi((double)m / (double)k, s_cut);
            if (label_hits) label_hits[r] = h;
        }
    }
}

// Max mode over few docs (D <= kKeepRowDocs): one thread per read scans its own row, where a wavefront
// per row would leave most lanes idle.
constexpr uint64_t kKeepRowDocs = 16;
__global__ void __launch_bounds__(256) filter_keep_max_row_kernel(const uint32_t* __restrict__ hits,
                                                                  const uint64_t* __restrict__ nk, uint64_t n,
                                                                  uint64_t D, uint64_t label,
                                                                  const uint8_t* __restrict__ mask, FilterCuts cuts,
                                                                  uint8_t* __restrict__ keep,
                                                                  uint32_t* __restrict__ label_hits) {
    __shared__ double s_cut[kFilterCuts];
    for (int i = threadIdx.x; i < kFilterCuts; i += blockDim.x) s_cut[i] = cuts.c[i];
    __syncthreads();
    for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t* row = hits + r * D;
        uint32_t m = 0;
        for (uint64_t d = 0; d < D; ++d)
            if (!mask || mask[d]) m = max(m, row[d]);
        const uint32_t h = row[label];
        const uint64_t k = nk[r];
        keep[r] = k != 0 && filter_centi((double)h / (double)k, s_cut) == filter_centi((double)m / (double)k, s_cut);
        if (label_hits) label_hits[r] = h;
    }
}

// ------------------------------------------------------------------ compaction
// An exclusive scan of (kept, kept length) over the reads in three launches, so the result does not
// depend on the order in which blocks run: per-block sums of kCompactBlock reads, one block that scans
// those sums, and the blocks again, each scanning its own reads from its base.
constexpr int kCompactThreads = 256;
constexpr int kCompactPer = kCompactBlock / kCompactThreads;  // consecutive reads per thread

// Exclusive scan of (c, l) over the block's threads in thread order; tot_*: the block's sums.
// s_c / s_l: one entry per wave.  Ends with a barrier, so the LDS is free again on return.
template <int WAVES>
__device__ __forceinline__ void block_scan(uint32_t& c, uint64_t& l, uint32_t& tot_c, uint64_t& tot_l, uint32_t* s_c,
                                           uint64_t* s_l) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t ic = c;
    uint64_t il = l;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t tc = __shfl_up(ic, o, 64);
        const uint64_t tl = __shfl_up((unsigned long long)il, o, 64);
        if (lane >= o) {
            ic += tc;
            il += tl;
        }
    }
    if (lane == 63) {
        s_c[w] = ic;
        s_l[w] = il;
    }
    __syncthreads();
    uint32_t bc = 0;
    uint64_t bl = 0;
    tot_c = 0;
    tot_l = 0;
#pragma unroll
    for (int j = 0; j < WAVES; ++j) {
        if (j < w) {
            bc += s_c[j];
            bl += s_l[j];
        }
        tot_c += s_c[j];
        tot_l += s_l[j];
    }
    c = bc + ic - c;
    l = bl + il - l;
    __syncthreads();
}

// The thread's reads [i0, i0 + kCompactPer) clipped to n: which are kept and how long they are.
__device__ __forceinline__ void compact_load(const uint8_t* __restrict__ keep, const uint64_t* __restrict__ offs,
                                             uint64_t n, uint64_t i0, bool (&kp)[kCompactPer],
                                             uint64_t (&len)[kCompactPer], uint32_t& c, uint64_t& l) {
    c = 0;
    l = 0;
#pragma unroll
    for (int j = 0; j < kCompactPer; ++j) {
        const uint64_t i = i0 + j;
        kp[j] = i < n && keep[i] != 0;
        len[j] = kp[j] ? offs[i + 1] - offs[i] : 0;
        c += kp[j];
        l += len[j];
    }
}

__global__ void __launch_bounds__(kCompactThreads) compact_sums_kernel(const uint8_t* __restrict__ keep,
                                                                       const uint64_t* __restrict__ offs, uint64_t n,
                                                                       uint64_t* __restrict__ blk_len,
                                                                       uint32_t* __restrict__ blk_cnt) {
    __shared__ uint32_t s_c[kCompactThreads / 64];
    __shared__ uint64_t s_l[kCompactThreads / 64];
    bool kp[kCompactPer];
    uint64_t len[kCompactPer];
    uint32_t c, tc;
    uint64_t l, tl;
    compact_load(keep, offs, n, blockIdx.x * (uint64_t)kCompactBlock + threadIdx.x * kCompactPer, kp, len, c, l);
    block_scan<kCompactThreads / 64>(c, l, tc, tl, s_c, s_l);
    if (threadIdx.x == 0) {
        blk_cnt[blockIdx.x] = tc;
        blk_len[blockIdx.x] = tl;
    }
}

// One block: the per-block sums become their exclusive prefixes (in place), tile by tile with a carry;
// then counts = {m, kept bytes} and the closing entry out_offs[m].
constexpr int kScanThreads = 1024;
__global__ void __launch_bounds__(kScanThreads) compact_scan_blocks_kernel(uint64_t* __restrict__ blk_len,
                                                                          uint32_t* __restrict__ blk_cnt, uint64_t nb,
                                                                          uint64_t* __restrict__ out_offs,
                                                                          uint64_t* __restrict__ counts) {
    __shared__ uint32_t s_c[kScanThreads / 64];
    __shared__ uint64_t s_l[kScanThreads / 64];
    uint64_t carry_c = 0, carry_l = 0;  // m < 2^32, kept in 64 bits with the bytes
    for (uint64_t t0 = 0; t0 < nb; t0 += kScanThreads) {
        const uint64_t i = t0 + threadIdx.x;
        uint32_t c = i < nb ? blk_cnt[i] : 0, tc;
        uint64_t l = i < nb ? blk_len[i] : 0, tl;
        block_scan<kScanThreads / 64>(c, l, tc, tl, s_c, s_l);
        if (i < nb) {
            blk_cnt[i] = (uint32_t)(carry_c + c);
            blk_len[i] = carry_l + l;
        }
        carry_c += tc;
        carry_l += tl;
    }
    if (threadIdx.x == 0) {
        counts[0] = carry_c;
        counts[1] = carry_l;
        out_offs[carry_c] = carry_l;
    }
}

__global__ void __launch_bounds__(kCompactThreads) compact_scatter_kernel(const uint8_t* __restrict__ keep,
                                                                          const uint64_t* __restrict__ offs, uint64_t n,
                                                                          const uint64_t* __restrict__ blk_len,
                                                                          const uint32_t* __restrict__ blk_cnt,
                                                                          uint32_t* __restrict__ index,
                                                                          uint64_t* __restrict__ out_offs) {
    __shared__ uint32_t s_c[kCompactThreads / 64];
    __shared__ uint64_t s_l[kCompactThreads / 64];
    bool kp[kCompactPer];
    uint64_t len[kCompactPer];
    uint32_t c, tc;
    uint64_t l, tl;
    const uint64_t i0 = blockIdx.x * (uint64_t)kCompactBlock + threadIdx.x * kCompactPer;
    compact_load(keep, offs, n, i0, kp, len, c, l);
    block_scan<kCompactThreads / 64>(c, l, tc, tl, s_c, s_l);
    uint64_t pos = (uint64_t)blk_cnt[blockIdx.x] + c;  // < m: only kept reads store
    uint64_t off = blk_len[blockIdx.x] + l;
#pragma unroll
    for (int j = 0; j < kCompactPer; ++j) {
        if (kp[j]) {
            index[pos] = (uint32_t)(i0 + j);
            out_offs[pos] = off;
            ++pos;
            off += len[j];
        }
    }
}

}  // namespace

// ------------------------------------------------------------------ launchers
hipError_t launch_filter_keep(const uint32_t* hits, const uint64_t* nk, uint64_t n, uint64_t D, uint64_t label,
                              const uint8_t* mask, int c_min, uint8_t* keep, uint32_t* label_hits, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const FilterCuts& cuts = filter_cuts();
    // one column is its own maximum: max mode keeps every read with k-mers, as c_min = 0 does
    if (c_min < 0 && D == 1) c_min = 0;
    if (c_min >= 0)
        filter_keep_threshold_kernel<<<grid_for(n, 256, 4096), 256, 0, s>>>(hits, nk, n, D, label, cuts.c[c_min], keep,
                                                                          label_hits);
    else if (D <= kKeepRowDocs)
        filter_keep_max_row_kernel<<<grid_for(n, 256, 4096), 256, 0, s>>>(hits, nk, n, D, label, mask, cuts, keep,
                                                                        label_hits);
    else
        filter_keep_max_kernel<<<grid_for(n, 4, 16384), 256, 0, s>>>(hits, nk, n, D, label, mask, cuts, keep,
                                                                    label_hits);
    return hipGetLastError();
}

hipError_t launch_filter_compact(const uint8_t* keep, const uint64_t* offs, uint64_t n, uint32_t* index,
                                 uint64_t* out_offs, uint64_t* counts, hipStream_t s) {
    const uint64_t nb = (n + kCompactBlock - 1) / kCompactBlock;
    // the per-block sums: stream-ordered scratch, so calls on different streams never share it
    void* tmp = nullptr;
    if (nb)
        if (hipError_t e = hipMallocAsync(&tmp, nb * 16, s)) return e;
    uint64_t* blk_len = static_cast<uint64_t*>(tmp);
    uint32_t* blk_cnt = reinterpret_cast<uint32_t*>(blk_len + nb);
    if (nb) compact_sums_kernel<<<(unsigned)nb, kCompactThreads, 0, s>>>(keep, offs, n, blk_len, blk_cnt);
    compact_scan_blocks_kernel<<<1, kScanThreads, 0, s>>>(blk_len, blk_cnt, nb, out_offs, counts);
    if (nb) compact_scatter_kernel<<<(unsigned)nb, kCompactThreads, 0, s>>>(keep, offs, n, blk_len, blk_cnt, index, out_offs);
    const hipError_t launched = hipGetLastError();
    if (nb)
        if (hipError_t e = hipFreeAsync(tmp, s)) return e;
    return launched;
}

}  // namespace xs
