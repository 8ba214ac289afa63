// xs_mlst_chunks.hip — MLST typing of contigs on the device: the splitter, the chunk-score
// accumulation and the per-record top allele.
//
// The reference cuts a record of 10 kbp and more into chunks of about one allele length per locus
// (sequence_splitter, probabilistic_filter_mlst_model.py:382-426), searches every chunk, keeps the
// chunk scores > 50 and sums them per allele (:236-256); the first allele of the stable sort by
// -sum is the call.  Here the chunk texts are cut on the device from the reads already in HBM
// (mlst_split_kernel), probed like reads, and their rows reduced in two steps that leave nothing
// for the host: one pass of integer atomics per (record, allele) (mlst_chunk_acc_kernel), then one
// wave per record over its D accumulators (mlst_owner_top_kernel).  The order of the reference's
// dict (first passing chunk, then rank in that chunk's COBS order) is a 64-bit key,
// chunk << 32 | (0xFFFFFFFF - count), whose minimum does not depend on the order of arrival.
#include "xs_device.h"

namespace xs {

namespace {

constexpr uint64_t kPadBytes = 64;  // zero bytes behind the last chunk (xs_host.h kPad)

// the last element of begin[0 .. n] (at `stride` words) that is <= row: the run or owner holding it
__device__ __forceinline__ uint64_t holder_of(const uint64_t* __restrict__ begin, uint32_t stride, uint64_t n,
                                              uint64_t row) {
    uint64_t lo = 0, hi = n;  // begin[lo] <= row < begin[hi]
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (begin[mid * stride] <= row) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace

// Runs of whole records, one block: tiles of 256 records, chunk and byte counts scanned through LDS.
__global__ void __launch_bounds__(256) mlst_runs_kernel(const uint64_t* __restrict__ offs,
                                                        const uint32_t* __restrict__ index, uint64_t m, uint64_t w,
                                                        uint32_t k, uint64_t scale10, uint64_t scale100,
                                                        MlstChunkRun* __restrict__ runs,
                                                        uint64_t* __restrict__ owner_begin) {
    __shared__ uint64_t sc[256], sb[256];
    __shared__ uint64_t base_c, base_b;
    const uint32_t t = threadIdx.x;
    if (t == 0) base_c = base_b = 0;
    __syncthreads();
    for (uint64_t e0 = 0; e0 < m; e0 += 256) {
        const uint64_t e = e0 + t;
        uint64_t src = 0, n = 0, W = w, rec = 0, c = 0, b = 0;
        if (e < m) {
            rec = index[e];
            src = offs[rec];
            n = offs[rec + 1] - src;
            W = mlst_chunk_width(n, w, scale10, scale100);
            const MlstRecGeom g = mlst_rec_geom(n, W, k);
            c = g.chunks;
            b = g.bytes;
        }
        sc[t] = c;
        sb[t] = b;
        __syncthreads();
        for (uint32_t d = 1; d < 256; d <<= 1) {  // inclusive scan
            const uint64_t ac = t >= d ? sc[t - d] : 0, ab = t >= d ? sb[t - d] : 0;
            __syncthreads();
            sc[t] += ac;
            sb[t] += ab;
            __syncthreads();
        }
        if (e < m) {
            const uint64_t row0 = base_c + sc[t] - c, out = base_b + sb[t] - b;
            runs[e] = MlstChunkRun{row0, src, n, W, 0, out, rec, 0};
            owner_begin[e] = row0;
        }
        __syncthreads();
        if (t == 255) {
            base_c += sc[255];
            base_b += sb[255];
        }
        __syncthreads();
    }
    if (t == 0) {
        runs[m] = MlstChunkRun{base_c, 0, 0, 0, 0, base_b, 0, 0};
        owner_begin[m] = base_c;
    }
}

// One wave per chunk: its one or two source segments (the chunk's window of the record, then for
// the repeated tail the record's last k - 1 bytes again) copied byte-wise, lanes on consecutive
// bytes.  Sources are unaligned and destinations packed, so no wider access is aligned on both sides.
__global__ void __launch_bounds__(256) mlst_split_kernel(const uint8_t* __restrict__ seqs,
                                                         const MlstChunkRun* __restrict__ runs, uint64_t n_runs,
                                                         uint64_t nc, uint32_t k, uint8_t* __restrict__ text,
                                                         uint64_t* __restrict__ chunk_offs) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t c = wave; c < nc; c += waves) {
        const MlstChunkRun r = runs[holder_of(&runs->row0, kMlstRunWords, n_runs, c)];
        const MlstRecGeom g = mlst_rec_geom(r.n, r.W, k);
        const uint64_t j = r.j0 + (c - r.row0);
        const uint64_t len = mlst_chunk_len(g, r.n, r.W, k, j);
        const uint64_t out = r.out + (c - r.row0) * r.W;  // every chunk before this one in the run is W bytes
        const uint64_t start = j * g.S, avail = r.n - start;  // bytes past `avail` repeat the record's tail
        const uint8_t* src = seqs + r.src;
        for (uint64_t b = lane; b < len; b += 64)
            text[out + b] = b < avail ? src[start + b] : src[r.n - (k - 1) + (b - avail)];
        if (lane == 0) chunk_offs[c] = out;
        if (c + 1 == nc) {
            if (lane == 0) chunk_offs[nc] = out + len;
            if (lane < kPadBytes) text[out + len + lane] = 0;
        }
    }
}

// The matrix as one flat array: counts up to the first 16-byte boundary, 16-byte loads, the rest.
__global__ void __launch_bounds__(256) mlst_chunk_acc_kernel(const uint32_t* __restrict__ hits, uint64_t total,
                                                             uint64_t D, const uint64_t* __restrict__ begin,
                                                             uint32_t stride, uint64_t n_owners, uint32_t threshold,
                                                             uint64_t chunk_base, unsigned long long* __restrict__ sum,
                                                             unsigned long long* __restrict__ key) {
    const uint64_t t0 = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    const uint64_t nt = (uint64_t)gridDim.x * blockDim.x;
    auto take = [&](uint64_t i, uint32_t v) {
        if (v <= threshold) return;
        const uint64_t c = i / D, d = i - c * D;
        if (c < begin[0] || c >= begin[n_owners * stride]) return;  // a row no owner holds
        const uint64_t o = holder_of(begin, stride, n_owners, c) * D + d;
        atomicAdd(&sum[o], (unsigned long long)v);
        atomicMin(&key[o], (unsigned long long)(((chunk_base + c) << 32) | (0xFFFFFFFFu - v)));
    };
    const uint64_t mis = (reinterpret_cast<uintptr_t>(hits) >> 2) & 3u;
    const uint64_t head = min((uint64_t)((4u - mis) & 3u), total);
    const uint64_t nvec = (total - head) >> 2, tail0 = head + 4 * nvec;
    if (t0 < head) take(t0, hits[t0]);
    const uint4* body = reinterpret_cast<const uint4*>(hits + head);
    for (uint64_t i = t0; i < nvec; i += nt) {
        const uint4 v = body[i];
        const uint64_t e = head + 4 * i;
        take(e, v.x);
        take(e + 1, v.y);
        take(e + 2, v.z);
        take(e + 3, v.w);
    }
    if (tail0 + t0 < total) take(tail0 + t0, hits[tail0 + t0]);
}

namespace {

// one lane's best (sum, key, doc) and the docs holding its largest sum; sum == 0: nothing qualifies
struct LaneBest {
    uint64_t s = 0, key = ~0ull;
    uint32_t doc = kMlstNone, cnt = 0;
    __device__ __forceinline__ void take(uint64_t v, uint64_t kk, uint32_t d) {
        if (v == 0) return;
        if (v > s) {
            s = v;
            key = kk;
            doc = d;
            cnt = 1;
        } else if (v == s) {
            ++cnt;
            if (kk < key || (kk == key && d < doc)) {
                key = kk;
                doc = d;
            }
        }
    }
};

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int o) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    return ((uint64_t)hi << 32) | lo;
}

}  // namespace

// One wave per owner.  Its two rows of D 64-bit values start 8-byte aligned: a head of 0-1 values
// up to the 16-byte boundary, a body of 16-byte loads (lane i takes docs 2i, 2i + 1), a tail of 0-1.
__global__ void __launch_bounds__(256) mlst_owner_top_kernel(const unsigned long long* __restrict__ sum,
                                                             const unsigned long long* __restrict__ key,
                                                             uint64_t n_owners, uint64_t D,
                                                             const uint64_t* __restrict__ rec, uint32_t rec_stride,
                                                             uint32_t* __restrict__ top,
                                                             uint32_t* __restrict__ top_score,
                                                             uint32_t* __restrict__ n_tied, uint64_t out_stride) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t o = wave; o < n_owners; o += waves) {
        const unsigned long long* srow = sum + o * D;
        const unsigned long long* krow = key + o * D;
        // sum and key are offset alike from 16-byte aligned bases only if the caller made them so: peel by each
        const uint32_t head = (uint32_t)min((uint64_t)((reinterpret_cast<uintptr_t>(srow) >> 3) & 1u), D);
        const bool kvec = ((reinterpret_cast<uintptr_t>(krow + head)) & 15u) == 0;
        const uint32_t nvec = (uint32_t)((D - head) >> 1);
        const uint32_t tail0 = head + 2u * nvec;
        LaneBest t;
        if (lane < head) t.take(srow[lane], krow[lane], lane);
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
            t.take(sv.x, kv.x, d);
            t.take(sv.y, kv.y, d + 1);
        }
        if (tail0 + lane < D) t.take(srow[tail0 + lane], krow[tail0 + lane], tail0 + lane);
        // wave: the largest sum; over its lanes the docs holding it and the lowest key; over those the lowest doc
        uint64_t ws = t.s;
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) ws = max(ws, shfl_xor64(ws, x));
        const bool in = t.cnt && t.s == ws;
        uint32_t c = in ? t.cnt : 0;
        uint64_t wk = in ? t.key : ~0ull;
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) {
            c += (uint32_t)__shfl_xor((int)c, x, 64);
            wk = min(wk, shfl_xor64(wk, x));
        }
        uint32_t a = (in && t.key == wk) ? t.doc : kMlstNone;
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) a = min(a, (uint32_t)__shfl_xor((int)a, x, 64));
        if (lane == 0) {
            const uint64_t w = (rec ? rec[o * rec_stride] : o) * out_stride;
            top[w] = ws ? a : kMlstNone;
            top_score[w] = (uint32_t)ws;
            if (n_tied) n_tied[w] = ws ? c : 0;
        }
    }
}

__global__ void __launch_bounds__(256) mlst_scatter_rows_kernel(const uint32_t* __restrict__ index, uint64_t m,
                                                                uint64_t cols, const uint32_t* __restrict__ src0,
                                                                const uint32_t* __restrict__ src1,
                                                                const uint32_t* __restrict__ src2,
                                                                uint32_t* __restrict__ dst0,
                                                                uint32_t* __restrict__ dst1,
                                                                uint32_t* __restrict__ dst2) {
    const uint64_t total = m * cols;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t j = i / cols, c = i - j * cols;
        const uint64_t w = (uint64_t)index[j] * cols + c;
        dst0[w] = src0[i];
        dst1[w] = src1[i];
        if (dst2) dst2[w] = src2[i];
    }
}

hipError_t launch_mlst_runs(const uint64_t* offs, const uint32_t* index, uint64_t m, uint64_t w, uint32_t k,
                            uint64_t scale10, uint64_t scale100, MlstChunkRun* runs, uint64_t* owner_begin,
                            hipStream_t s) {
    mlst_runs_kernel<<<1, 256, 0, s>>>(offs, index, m, w, k, scale10, scale100, runs, owner_begin);
    return hipGetLastError();
}

hipError_t launch_mlst_split(const uint8_t* seqs, const MlstChunkRun* runs, uint64_t n_runs, uint64_t nc, uint32_t k,
                             uint8_t* text, uint64_t* chunk_offs, hipStream_t s) {
    if (nc == 0) {
        hipError_t e = hipMemsetAsync(chunk_offs, 0, 8, s);
        return e != hipSuccess ? e : hipMemsetAsync(text, 0, kPadBytes, s);
    }
    mlst_split_kernel<<<grid_for(nc, 4, 16384), 256, 0, s>>>(seqs, runs, n_runs, nc, k, text, chunk_offs);
    return hipGetLastError();
}

hipError_t launch_mlst_chunk_acc(const uint32_t* hits, uint64_t nc, uint64_t D, const uint64_t* begin,
                                 uint32_t stride, uint64_t n_owners, uint32_t threshold, uint64_t chunk_base,
                                 unsigned long long* sum, unsigned long long* key, hipStream_t s) {
    if (nc == 0 || D == 0 || n_owners == 0) return hipSuccess;
    mlst_chunk_acc_kernel<<<grid_for((nc * D + 3) / 4, 256, 4096), 256, 0, s>>>(hits, nc * D, D, begin, stride,
                                                                                  n_owners, threshold, chunk_base, sum,
                                                                                  key);
    return hipGetLastError();
}

hipError_t launch_mlst_owner_top(const unsigned long long* sum, const unsigned long long* key, uint64_t n_owners,
                                 uint64_t D, const uint64_t* rec, uint32_t rec_stride, uint32_t* top,
                                 uint32_t* top_score, uint32_t* n_tied, uint64_t out_stride, hipStream_t s) {
    if (n_owners == 0 || D == 0) return hipSuccess;
    mlst_owner_top_kernel<<<grid_for(n_owners, 4, 16384), 256, 0, s>>>(sum, key, n_owners, D, rec, rec_stride, top,
                                                                         top_score, n_tied, out_stride);
    return hipGetLastError();
}

hipError_t launch_mlst_scatter_rows(const uint32_t* index, uint64_t m, uint64_t cols, const uint32_t* src0,
                                    const uint32_t* src1, const uint32_t* src2, uint32_t* dst0, uint32_t* dst1,
                                    uint32_t* dst2, hipStream_t s) {
    if (m == 0 || cols == 0) return hipSuccess;
    mlst_scatter_rows_kernel<<<grid_for(m * cols, 256, 4096), 256, 0, s>>>(index, m, cols, src0, src1, src2, dst0,
                                                                            dst1, dst2);
    return hipGetLastError();
}

}  // namespace xs
