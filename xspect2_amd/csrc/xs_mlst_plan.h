// xs_mlst_plan.h — the host's plan of a contig typing call (xs_mlst.cpp): which records are long, and
// how every locus' chunks are cut into ranges of runs.  Arithmetic on the records' offsets alone: no
// HIP runtime call and no bank handle, so the host sanitizer driver (tools/asan) includes it as it is.
// It decides which device bytes the splitter writes.
#pragma once
#include "../../include/xspect_hip.h"

#include <algorithm>

#include "xs_internal.h"

namespace xs {

constexpr xs_mlst_chunk_rule_t kReferenceRule{10000, 1000000, 10000000, 50, 0};

inline int chunk_rule_check(const xs_mlst_chunk_rule_t* rule, xs_mlst_chunk_rule_t* out) {
    *out = rule ? *rule : kReferenceRule;
    if (out->scale10_len > out->scale100_len) return fail(XS_ERR_ARG, "scale10_len must be <= scale100_len");
    return XS_OK;
}

// The rule, locus width and k of xs_mlst_split_size / xs_mlst_split_device.
inline int split_args_check(const xs_mlst_chunk_rule_t* rule, uint64_t width, uint32_t k, xs_mlst_chunk_rule_t* out) {
    if (int rc = chunk_rule_check(rule, out)) return rc;
    if (k == 0 || width < k) return fail(XS_ERR_ARG, "width must be >= k >= 1");
    if (out->long_len < k) return fail(XS_ERR_ARG, "long_len must be >= k = %u", k);
    return XS_OK;
}

// The records by kind: the long ones (long_len bytes and more), and the runs [first, end) of
// consecutive short ones with their records and bytes in all.  ho: the n + 1 host offsets.
struct RecordKinds {
    std::vector<uint64_t> longs;
    std::vector<std::pair<uint64_t, uint64_t>> short_runs;
    uint64_t n_short = 0, short_bytes = 0;
};
inline RecordKinds classify_records(const uint64_t* ho, uint64_t n, uint64_t long_len) {
    RecordKinds kinds;
    for (uint64_t r = 0, run = 0; r <= n; ++r) {
        const bool is_long = r < n && ho[r + 1] - ho[r] >= long_len;
        if (r == n || is_long) {
            if (r > run) {
                kinds.short_runs.emplace_back(run, r);
                kinds.n_short += r - run;
                kinds.short_bytes += ho[r] - ho[run];
            }
            run = r + 1;
            if (is_long) kinds.longs.push_back(r);
        }
    }
    return kinds;
}

// One range of one locus: runs [run0, run0 + n_runs) of the call's run array (a sentinel follows them).
struct ChunkRange {
    uint64_t run0, n_runs, nc, bytes, chunk_base;
    bool carry_in, carry_out;  // its first run continues a record / its last run's record goes on
};

// The ranges of one locus appended to `ranges`, their runs to `runs`.  ho: the reads' host offsets.
inline void cut_chunk_ranges(const std::vector<uint64_t>& longs, const uint64_t* ho, uint64_t w, uint32_t k,
                             const xs_mlst_chunk_rule_t& rule, uint64_t row_cap, uint64_t text_cap,
                             std::vector<MlstChunkRun>* runs, std::vector<ChunkRange>* ranges) {
    uint64_t run0 = runs->size(), cu = 0, bu = 0, base = 0;
    bool carry_in = false;
    auto close = [&](bool carry_out) {
        runs->push_back(MlstChunkRun{cu, 0, 0, 0, 0, bu, 0, 0});
        ranges->push_back(ChunkRange{run0, runs->size() - 1 - run0, cu, bu, base, carry_in, carry_out});
        base += cu;
        run0 = runs->size();
        cu = bu = 0;
        carry_in = carry_out;
    };
    for (uint64_t rec : longs) {
        const uint64_t n = ho[rec + 1] - ho[rec];
        const uint64_t W = mlst_chunk_width(n, w, rule.scale10_len, rule.scale100_len);
        const MlstRecGeom g = mlst_rec_geom(n, W, k);
        for (uint64_t j = 0; j < g.chunks;) {
            uint64_t fit = text_cap > bu ? (text_cap - bu) / W : 0;  // a record's last chunk may exceed W by k - 1
            if (cu == 0) fit = std::max<uint64_t>(fit, 1);           // a range takes at least one chunk
            uint64_t take = std::min({g.chunks - j, row_cap - cu, fit});
            // ... and that chunk is left to the next range where it would take one of several chunks over the cap
            const uint64_t last = mlst_chunk_len(g, n, W, k, g.chunks - 1);
            if (take && j + take == g.chunks && cu + take > 1 && bu + (take - 1) * W + last > text_cap) --take;
            if (take == 0) {
                close(j > 0);
                continue;
            }
            const bool to_end = j + take == g.chunks;
            const uint64_t nb = to_end ? (take - 1) * W + last : take * W;
            runs->push_back(MlstChunkRun{cu, ho[rec], n, W, j, bu, rec, 0});
            cu += take;
            bu += nb;
            j += take;
        }
    }
    if (cu) close(false);
}

}  // namespace xs
