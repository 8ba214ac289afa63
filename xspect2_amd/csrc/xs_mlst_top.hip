// xs_mlst_top.hip — per hit row, the top allele of an MLST locus on the device.
//
// The reference takes the first item of a locus' COBS result as the record's
// allele (probabilistic_filter_mlst_model.py:272-286); COBS orders by score
// descending, ties by doc index.  For a row of D counts that is
//   top = min{d : row[d] == max(row)},  top_score = max(row),
// and n_tied = |{d : row[d] == max(row)}| says how many alleles share it (an
// all-zero row: top 0, score 0, n_tied D).  Reduced here, the n x D matrix of a
// locus never leaves HBM: 12 bytes per (record, locus) go to the host.
//
// The pass is one stream over the matrix.  One wavefront per row; a row starts
// at byte r*D*4, 4-byte aligned only (D = 1430: rows alternate between 16- and
// 8-byte alignment), so each row is read as a head of 0-3 counts up to the next
// 16-byte boundary, a body of 16-byte loads (lane i takes counts 4i..4i+3), and
// a tail of 0-3 counts.
#include "xs_device.h"

namespace xs {

namespace {

// one lane's running (max, lowest doc holding it, docs holding it); cnt == 0: nothing seen yet
struct LaneTop {
    uint32_t m = 0, arg = 0xFFFFFFFFu, cnt = 0;
    __device__ __forceinline__ void take(uint32_t v, uint32_t d) {
        if (cnt == 0 || v > m) {
            m = v;
            arg = d;
            cnt = 1;
        } else if (v == m) {
            ++cnt;
            arg = min(arg, d);  // a lane meets the head, the body and the tail in that order, not by doc
        }
    }
};

}  // namespace

__global__ void __launch_bounds__(256) mlst_top_kernel(const uint32_t* __restrict__ hits, uint64_t n, uint64_t D,
                                                       uint32_t* __restrict__ top, uint32_t* __restrict__ top_score,
                                                       uint32_t* __restrict__ n_tied, uint64_t out_stride) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 6;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t r = wave; r < n; r += waves) {
        const uint32_t* row = hits + r * D;
        // counts before the first 16-byte boundary (all of a row shorter than that)
        const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(row) >> 2) & 3u;
        const uint32_t head = (uint32_t)min((uint64_t)((4u - mis) & 3u), D);
        const uint32_t nvec = (uint32_t)((D - head) >> 2);
        const uint32_t tail0 = head + 4u * nvec;
        LaneTop t;
        if (lane < head) t.take(row[lane], lane);
        const uint4* body = reinterpret_cast<const uint4*>(row + head);
        for (uint32_t i = lane; i < nvec; i += 64) {
            const uint4 v = body[i];
            const uint32_t d = head + 4u * i;
            t.take(v.x, d);
            t.take(v.y, d + 1);
            t.take(v.z, d + 2);
            t.take(v.w, d + 3);
        }
        if (tail0 + lane < D) t.take(row[tail0 + lane], tail0 + lane);
        // wave: the maximum, then over the lanes that hold it the lowest doc and the sum of the counts
        uint32_t wm = t.m;  // a lane that saw nothing holds 0, below or equal to every count
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) wm = max(wm, (uint32_t)__shfl_xor((int)wm, o, 64));
        uint32_t c = (t.cnt && t.m == wm) ? t.cnt : 0;
        uint32_t a = c ? t.arg : 0xFFFFFFFFu;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            c += (uint32_t)__shfl_xor((int)c, o, 64);
            a = min(a, (uint32_t)__shfl_xor((int)a, o, 64));
        }
        if (lane == 0) {
            const uint64_t o = r * out_stride;
            top[o] = a;
            top_score[o] = wm;
            if (n_tied) n_tied[o] = c;
        }
    }
}

hipError_t launch_mlst_top(const uint32_t* hits, uint64_t n, uint64_t D, uint32_t* top, uint32_t* top_score,
                           uint32_t* n_tied, uint64_t out_stride, hipStream_t s) {
    if (n == 0 || D == 0) return hipSuccess;
    mlst_top_kernel<<<grid_for(n, 4, 16384), 256, 0, s>>>(hits, n, D, top, top_score, n_tied, out_stride);
    return hipGetLastError();
}

}  // namespace xs
