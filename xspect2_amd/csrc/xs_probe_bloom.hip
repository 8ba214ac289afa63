// xs_probe_bloom.hip — rbloom gather probe: one wavefront per unit, one lane per k-mer, K random
// dword loads from the filter (the direct path of genus banks; xs_probe_bloompart.hip is the partitioned one).
#include "xs_direct.h"

namespace xs {

// ------------------------------------------------------------------ rbloom probe
// Filter bits tested before the rest: 2 measured fastest for member-heavy
// and foreign-heavy reads alike (all 7 at once: 15.69 against 13.43 ms per
// config-2 step).
constexpr int kBloomSplit = 2;
// All K bit indices first, then all K dword loads in flight at once (the
// reference stops at the first zero bit; the answer is the same).
// Returns bit 0: member; bit 1: the second load phase ran.
template <int KT, int KB, int SPLIT>
__device__ __forceinline__ uint32_t bloom_member(const Kmer& c, uint32_t k, const BloomView& bv) {
    constexpr int NK = KB ? KB : (int)kMaxHashes;
    const uint32_t K = KB ? KB : bv.K;
    uint64_t sl = xxh3_kmer<KT>(c, k), sh = 0;
    uint64_t idx[NK];
#pragma unroll
    for (int j = 0; j < NK; ++j) {
        if ((uint32_t)j < K) {
            lcg_step(sl, sh);
            idx[j] = fastmod(sh, bv.mbits, bv.magic);
        }
    }
    // The first SPLIT bits decide most non-members (rbloom stops at the
    // first zero bit); the other loads go out only for lanes still in.
    // SPLIT = 0: all K loads at once.
    uint32_t all = 1;
#pragma unroll
    for (int j = 0; j < NK; ++j)
        if ((uint32_t)j < K && (SPLIT == 0 || j < SPLIT)) all &= bv.bits[idx[j] >> 5] >> (idx[j] & 31);
    uint32_t phase2 = 0;
    if (SPLIT != 0 && (all & 1u) && (uint32_t)SPLIT < K) {
        phase2 = 2u;
#pragma unroll
        for (int j = SPLIT; j < NK; ++j)
            if ((uint32_t)j < K) all &= bv.bits[idx[j] >> 5] >> (idx[j] & 31);
    }
    return (all & 1u) | phase2;
}

template <int KT, int KB, int SPLIT>
__global__ void __launch_bounds__(kProbeThreads) probe_bloom_kernel(ReadView rv, BloomView bv,
                                                                    uint32_t* __restrict__ hits,
                                                                    uint64_t* __restrict__ partials) {
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int wpb = blockDim.x >> 6;
    __shared__ uint64_t s_hits[kProbeThreads / kWave], s_kmers[kProbeThreads / kWave];
    const uint32_t k = KT ? KT : rv.k;
    const uint32_t step = rv.step;
    uint64_t hit_total = 0, kmer_total = 0, rows_total = 0;

    walk_units(rv, lane, k, step, [&](const Unit& n) {
        uint32_t c_unit = 0;
        for (uint32_t tb = 0; tb < n.cnt; tb += 64) {
            bool in = false, again = false;
            if (tb + lane < n.cnt) {
                Kmer c;
                kmer_at<KT, kKmerBio>(rv, n.o0, n.len, (n.t0 + tb + lane) * step, k, c);
                const uint32_t res = bloom_member<KT, KB, SPLIT>(c, k, bv);
                in = res & 1u;
                again = (res & 2u) != 0;
            }
            c_unit += (uint32_t)__popcll(__ballot(in));
            if (bv.rows_read) {
                const uint32_t K = KB ? KB : bv.K;
                const uint32_t first = SPLIT == 0 || (uint32_t)SPLIT >= K ? K : (uint32_t)SPLIT;
                rows_total += (uint64_t)__popcll(__ballot(tb + lane < n.cnt)) * first +
                              (uint64_t)__popcll(__ballot(again)) * (K - first);
            }
        }
        kmer_total += n.cnt;
        hit_total += c_unit;
        if (hits && lane == 0) store_hit(hits, n.r, c_unit, n.whole());
    });
    if (bv.rows_read && lane == 0 && rows_total)
        atomicAdd(reinterpret_cast<unsigned long long*>(bv.rows_read), (unsigned long long)rows_total);
    if (partials) {
        if (lane == 0) { s_hits[wid] = hit_total; s_kmers[wid] = kmer_total; }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t a = 0, b = 0;
            for (int w = 0; w < wpb; ++w) { a += s_hits[w]; b += s_kmers[w]; }
            partials[blockIdx.x * 2ull] = a;
            partials[blockIdx.x * 2ull + 1] = b;
        }
    }
}

// ------------------------------------------------------------------ launch
int probe_grid_bloom() {
    static std::atomic<int> cache{0};
    return cached_grid(cache, [] { return resident_grid(probe_bloom_kernel<21, 7, kBloomSplit>, kProbeThreads, 0); });
}

hipError_t launch_probe_bloom(const ReadView& rv, const BloomView& bv, uint32_t* hits,
                              uint64_t* partials, int blocks, hipStream_t s, const char** kernel) {
    using BloomFn = void (*)(ReadView, BloomView, uint32_t*, uint64_t*);
    static const struct { const char* name; BloomFn fn; } kBloomKernels[2] = {
        {"bloom<21,7>", probe_bloom_kernel<21, 7, kBloomSplit>}, {"bloom<0,0>", probe_bloom_kernel<0, 0, kBloomSplit>}};
    const auto& e = kBloomKernels[rv.k == 21 && bv.K == 7 ? 0 : 1];
    if (kernel) *kernel = e.name;
    e.fn<<<blocks, kProbeThreads, 0, s>>>(rv, bv, hits, partials);
    return hipGetLastError();
}

}  // namespace xs
