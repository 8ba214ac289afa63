// xs_part.h — pieces shared by the partitioned probes (xs_probe_bloompart.hip,
// xs_probe_cobspart.hip): per-read k-mer counts and their scan give every
// sampled k-mer a global id; bucket blocks of consecutive ids are mapped to
// the reads they start in, stage those reads in LDS and find each k-mer's
// window there; partition starts are transposed from block-major to
// partition-major for the per-XCD lookup queues, from which the lookup waves
// take groups of bucket blocks and build each window's entry -> block map.
// The host side shares the partition-shift rule, the plan's common sizes, the
// lookup grid and the counts + scan launch.
#pragma once
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "xs_device.h"

namespace xs {

namespace {

constexpr int kTK = kPartKmers;  // k-mers per bucket block
constexpr int kBucketThreads = 512;
constexpr uint32_t kStageReads = 256;  // read offsets a bucket block keeps in LDS

__global__ void part_counts_kernel(const uint64_t* __restrict__ offs, uint64_t n, uint32_t k, uint32_t step,
                                   uint64_t* __restrict__ nkc) {
    for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r <= n;
         r += (uint64_t)gridDim.x * blockDim.x)
        nkc[r] = r < n ? num_kmers(offs[r + 1] - offs[r], k, step) : 0;
}

// Largest r in [lo, hi] with kofs[r] <= g (kofs non-decreasing, kofs[lo] <= g).
__device__ __forceinline__ uint64_t read_of(const uint64_t* __restrict__ kofs, uint64_t lo, uint64_t hi,
                                            uint64_t g) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (kofs[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// blk_read[b] = the read holding k-mer b*TK (the first k-mer of bucket block b).
template <int TK = kTK>
__global__ void part_map_kernel(const uint64_t* __restrict__ kofs, uint64_t n, uint32_t* __restrict__ blk_read) {
    for (uint64_t r = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; r < n;
         r += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t fb = (kofs[r] + TK - 1) / TK, lb = (kofs[r + 1] + TK - 1) / TK;
        for (uint64_t b = fb; b < lb; ++b) blk_read[b] = (uint32_t)r;
    }
}

// ---- bucket pass: the reads of a block ---------------------------------------------
// Reads lo .. hi hold the TK k-mers from g0 on: from the one holding k-mer g0 to the one
// holding the next block's first k-mer (or the last read).  Their k-mer and byte offsets
// (kofs / offs entries lo .. hi+1) go to LDS when they fit (returns true), so a k-mer
// costs one global load (its window) and every thread's windows are in flight together.
// Then s_map[i] = the block-local read of k-mer g0 + i, from each read's first k-mer marked
// and a block-wide max-scan.  BT threads; holds the block's first barrier, which also
// covers what the kernel cleared before the call.
template <int TK, int BT, class Scan>
__device__ __forceinline__ bool part_stage_reads(const ReadView& rv, const uint64_t* __restrict__ kofs, uint64_t g0,
                                                 uint64_t lo, uint64_t hi, uint64_t* s_kofs, uint64_t* s_offs,
                                                 uint32_t* s_map, typename Scan::TempStorage& scan_tmp) {
    constexpr int PER = TK / BT;  // k-mers per thread
    const int tid = threadIdx.x;
    const uint64_t nr = hi - lo + 2;
    const bool staged = nr <= kStageReads;
    if (staged) {
        for (uint32_t x = tid; x < nr; x += BT) {
            s_kofs[x] = kofs[lo + x];
            s_offs[x] = rv.offs[lo + x];
        }
        for (uint32_t i = tid; i < TK; i += BT) s_map[i] = 0;  // read 0 holds k-mer g0
    }
    __syncthreads();
    if (staged) {
        // reads 1 .. nr-2 start inside the block or after it; empty reads share a start
        // with the next read, and the max keeps the later one
        for (uint32_t x = 1 + tid; x + 1 < nr; x += BT) {
            const uint64_t st = s_kofs[x] - g0;
            if (st < (uint64_t)TK) atomicMax(&s_map[st], x);
        }
        __syncthreads();
        uint32_t mv[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) mv[q] = s_map[tid * PER + q];
        Scan(scan_tmp).InclusiveScan(mv, mv, hipcub::Max());
#pragma unroll
        for (int q = 0; q < PER; ++q) s_map[tid * PER + q] = mv[q];
        __syncthreads();
    }
    return staged;
}

// Where k-mer g0 + i lies: its read's first byte, the read's length, and the k-mer's
// position in the read; from LDS (staged) or by a binary search of kofs.
struct KmerWindow {
    uint64_t o0, len, pos;
};
__device__ __forceinline__ KmerWindow part_kmer_window(const ReadView& rv, const uint64_t* __restrict__ kofs,
                                                       bool staged, const uint32_t* s_map, const uint64_t* s_kofs,
                                                       const uint64_t* s_offs, uint64_t lo, uint64_t hi, uint64_t g0,
                                                       uint32_t i) {
    const uint64_t g = g0 + i;
    uint64_t kr, o0, o1;
    if (staged) {
        const uint32_t a = s_map[i];  // largest x with s_kofs[x] <= g
        kr = s_kofs[a];
        o0 = s_offs[a];
        o1 = s_offs[a + 1];
    } else {
        const uint64_t r = read_of(kofs, lo, hi, g);
        kr = kofs[r];
        o0 = rv.offs[r];
        o1 = rv.offs[r + 1];
    }
    return {o0, o1 - o0, (g - kr) * rv.step};
}

// Block-major partition starts (one coalesced row per bucket block) ->
// partition-major (the lookup reads 64 blocks' starts of one partition as one
// line), through a 64 x 64 LDS tile.
// Blocks b_begin .. b_end-1 (grid.x covers them in tiles of 64).
__global__ void __launch_bounds__(256) part_transpose_kernel(const uint16_t* __restrict__ tbm, uint32_t P1,
                                                             uint64_t tstride, uint16_t* __restrict__ tbl,
                                                             uint64_t b_begin, uint64_t b_end) {
    __shared__ uint16_t t[64][65];
    const uint64_t b0 = b_begin + (uint64_t)blockIdx.x * 64;
    const uint32_t p0 = blockIdx.y * 64;
    for (uint32_t x = threadIdx.x; x < 64 * 64; x += 256) {
        const uint32_t bi = x / 64, pi = x % 64;
        if (b0 + bi < b_end && p0 + pi < P1) t[bi][pi] = tbm[(b0 + bi) * P1 + p0 + pi];
    }
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < 64 * 64; x += 256) {
        const uint32_t pi = x / 64, bi = x % 64;
        if (b0 + bi < b_end && p0 + pi < P1) tbl[(p0 + pi) * tstride + b0 + bi] = t[bi][pi];
    }
}

// ---- lookup pass: groups of bucket blocks from a partition's queue ---------------
// u32 per lookup queue counter: each counter sits on its own 128-B line (a
// line's atomics are serialised at the memory side).
constexpr uint32_t kQStride = 32;  // u32 per queue counter

// The wave's next group of partition p (the same ticket in every lane).
__device__ __forceinline__ uint64_t part_take_group(uint32_t* qctr, uint64_t p, int lane) {
    uint32_t grp = 0;
    if (lane == 0) grp = atomicAdd(&qctr[p * kQStride], 1u);
    return (uint64_t)__builtin_amdgcn_readfirstlane(grp);
}

// One lane's bucket block b within its wave's group: the block's run of the partition holds
// len entries, entries pre .. pre + len - 1 of the group's total, and entry i of the group
// sits at position base + i (mod 2^32).  t0 / t1: the partition's and the next one's starts
// per block; stride: entries per block region.  A lane without a block (!valid) has len 0.
struct GroupRun {
    uint32_t pre, len, total, base;
};
__device__ __forceinline__ GroupRun part_group_run(const uint16_t* __restrict__ t0, const uint16_t* __restrict__ t1,
                                                   uint64_t b, bool valid, uint64_t stride, int lane) {
    uint32_t s = 0, len = 0;
    if (valid) {
        s = t0[b];
        len = (uint32_t)t1[b] - s;
    }
    uint32_t inc = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)inc, d, 64);
        if (lane >= d) inc += t;
    }
    const uint32_t pre = inc - len;
    const uint32_t total = (uint32_t)__shfl((int)inc, 63, 64);
    return {pre, len, total, (uint32_t)(b * stride + s) - pre};
}

// The entry -> base map of the group's entries w0 .. wend-1 in the wave's LDS row: each lane
// writes its block's base over its run's slots; then every entry can read its base.
__device__ __forceinline__ void part_window_bases(uint32_t* s_base, const GroupRun& g, uint32_t w0, uint32_t wend) {
    const uint32_t lo = max(g.pre, w0), hi = min(g.pre + g.len, wend);
    for (uint32_t x = lo; x < hi; ++x) s_base[x - w0] = g.base;
    __builtin_amdgcn_wave_barrier();
}

// Grid of a lookup kernel (256 threads): at most per_cu_cap workgroups per CU, in
// whole groups of 8 blocks (one per XCD).
template <class K>
static int part_lookup_grid(std::atomic<int>& cache, K kernel, int per_cu_cap) {
    return cached_grid(cache, [=] {
        int dev = 0, per_cu = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 768;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0) != hipSuccess || per_cu < 1)
            per_cu = 1;
        const int g = std::min(per_cu, per_cu_cap) * prop.multiProcessorCount;
        return g >= 8 ? g / 8 * 8 : 8;
    });
}

// ---- plans and launches ----------------------------------------------------------------
// Partition shift for a bank of `size` units (filter bits, COBS rows): 2^pref units per
// partition, halved down to 2^floor while that leaves fewer than 64 partitions (8 per XCD
// keep the XCDs evenly loaded), doubled while more than kPartMax.
static uint32_t part_shift(uint64_t size, uint32_t pref, uint32_t floor) {
    auto parts = [size](uint32_t s) { return (size + (1ull << s) - 1) >> s; };
    uint32_t s = pref;
    while (s > floor && parts(s) < 64) --s;
    while (parts(s) > kPartMax) ++s;
    return s;
}

// Upper bound of a call's sampled k-mers: >= sum of ceil((len-k+1)/step).
static uint64_t part_kbound(uint64_t n, uint64_t seq_bytes, uint32_t step) { return seq_bytes / step + n + 1; }

// The sizes every partitioned plan has: n reads, nblk bucket blocks, P partitions.
static void part_plan_sizes(PartSizes* z, uint64_t n, uint64_t kbound, uint64_t nblk, uint64_t P) {
    z->kbound = kbound;
    z->aux_bytes = (nblk + 1 + kQStride) * sizeof(uint32_t) + (size_t)P * kQStride * sizeof(uint32_t);
    z->nkc_bytes = (n + 1) * sizeof(uint64_t);
    size_t sb = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, sb, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)(n + 1));
    z->scan_bytes = sb;
}

// The queue counters of a plan of nblk blocks, behind blk_read in ws.aux (128-B aligned).
static uint32_t* part_queue_counters(const PartWs& ws, uint64_t nblk) {
    return ws.aux + (nblk + 1 + kQStride - 1) / kQStride * kQStride;
}

// Per-read k-mer counts and their exclusive scan: ws.kofs[r] = first k-mer id of read r.
static hipError_t part_launch_counts(const ReadView& rv, const PartWs& ws, hipStream_t s) {
    part_counts_kernel<<<grid_for(rv.n + 1, 256, 4096), 256, 0, s>>>(rv.offs, rv.n, rv.k, rv.step, ws.nkc);
    size_t sb = ws.scan_bytes;
    return hipcub::DeviceScan::ExclusiveSum(ws.scan_tmp, sb, ws.nkc, ws.kofs, (int)(rv.n + 1), s);
}

}  // namespace

}  // namespace xs
