// xs_filter.cpp — read filtering on the host side: the 101 rounding cuts, the threshold's mode, the
// keep decision over host rows (small calls) and the device entry points xs_filter_keep_device and
// xs_filter_compact_device.  xs_query_keep, which probes first, is in xs_query.cpp.
#include <cmath>

#include "xs_host.h"

using namespace xs;

namespace {

// cut[c], c >= 1: the smallest double >= (2c - 1) / 200, the point where round(x, 2) goes from
// (c - 1)/100 to c/100.  q = RN((2c - 1) / 200); the sign of the exact q * 200 - (2c - 1) (one fma)
// says on which side of that point q lies.  At an exact binary half the tie goes to the even
// centi-value, so an odd c starts one ulp later.
FilterCuts build_cuts() {
    FilterCuts t;
    t.c[0] = 0.0;
    for (int c = 1; c < kFilterCuts; ++c) {
        const double num = 2.0 * c - 1.0;
        double q = num / 200.0;
        const double side = std::fma(q, 200.0, -num);
        if (side < 0.0 || (side == 0.0 && (c & 1))) q = std::nextafter(q, 2.0);
        t.c[c] = q;
    }
    return t;
}

}  // namespace

const FilterCuts& xs::filter_cuts() {
    static const FilterCuts cuts = build_cuts();
    return cuts;
}

bool xs::filter_mode(double threshold, int* c_min) {
    if (threshold == -1.0) {
        *c_min = -1;
        return true;
    }
    if (!(threshold >= 0.0 && threshold <= 1.0)) return false;
    int c = 0;
    while ((double)c / 100.0 < threshold) ++c;  // ends at c <= 100: 100 / 100 >= threshold
    *c_min = c;
    return true;
}

void xs::filter_keep_rows(const uint32_t* rows, const uint64_t* nk, uint64_t n, uint64_t D, uint64_t label,
                          const uint8_t* mask, int c_min, uint8_t* keep, uint32_t* label_hits) {
    const double* cut = filter_cuts().c;
    for (uint64_t r = 0; r < n; ++r) {
        const uint32_t* row = rows + r * D;
        const uint32_t h = row[label];
        const uint64_t k = nk[r];
        if (label_hits) label_hits[r] = h;
        if (k == 0) {
            keep[r] = 0;
        } else if (c_min >= 0) {
            keep[r] = (double)h / (double)k >= cut[c_min];
        } else {
            uint32_t m = 0;
            for (uint64_t d = 0; d < D; ++d)
                if (!mask || mask[d]) m = std::max(m, row[d]);
            keep[r] = filter_centi((double)h / (double)k, cut) == filter_centi((double)m / (double)k, cut);
        }
    }
}

extern "C" {

int xs_filter_cuts(double* out, uint64_t n) {
    return xs::guard([&]() -> int {
        if (!out || n != (uint64_t)kFilterCuts) return fail(XS_ERR_ARG, "out must take %d cuts", kFilterCuts);
        memcpy(out, filter_cuts().c, sizeof(double) * kFilterCuts);
        return XS_OK;
    });
}

int xs_filter_keep_device(const uint32_t* d_hits, const uint64_t* d_num_kmers, uint64_t n, uint64_t num_docs,
                          uint64_t label_doc, const uint8_t* d_doc_mask, double threshold, uint8_t* d_keep,
                          uint32_t* d_label_hits, void* stream) {
    return xs::guard([&]() -> int {
        int c_min = 0;
        if (!filter_mode(threshold, &c_min)) return fail(XS_ERR_ARG, "threshold must be in [0, 1] or -1");
        if (label_doc >= num_docs) return fail(XS_ERR_ARG, "label_doc out of range");
        if ((!d_hits || !d_num_kmers || !d_keep) && n) return fail(XS_ERR_ARG, "null argument");
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (d_doc_mask) {  // in either mode: a masked label has no score (KeyError in the reference)
            uint8_t on = 0;
            HIPCHK(hipMemcpyAsync(&on, d_doc_mask + label_doc, 1, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (!on) return fail(XS_ERR_ARG, "label_doc is masked out");
        }
        HIPCHK(launch_filter_keep(d_hits, d_num_kmers, n, num_docs, label_doc, d_doc_mask, c_min, d_keep, d_label_hits,
                                  s));
        return XS_OK;
    });
}

int xs_filter_compact_device(const uint8_t* d_keep, const uint64_t* d_offsets, uint64_t n, uint32_t* d_index,
                             uint64_t* d_out_offsets, uint64_t* d_counts, void* stream) {
    return xs::guard([&]() -> int {
        if (!d_out_offsets || !d_counts || ((!d_keep || !d_offsets || !d_index) && n))
            return fail(XS_ERR_ARG, "null argument");
        if (n >> 32) return fail(XS_ERR_ARG, "at most 2^32-1 reads per call");
        HIPCHK(launch_filter_compact(d_keep, d_offsets, n, d_index, d_out_offsets, d_counts,
                                     static_cast<hipStream_t>(stream)));
        return XS_OK;
    });
}

}  // extern "C"
