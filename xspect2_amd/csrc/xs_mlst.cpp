// xs_mlst.cpp — the MLST entry points of the C ABI: chunk sums (xs_mlst_sum, xs_mlst_query), typing of
// reads (xs_mlst_type*) and of contigs (xs_mlst_type_contigs*, with the N best alleles xs_mlst_type_ranked*),
// and the splitter's and the reductions' pieces on their own.
// The probes are xs_query.cpp's (xs_query.h); the host's plan of a contig call is xs_mlst_plan.h.
#include "xs_mlst_plan.h"
#include "xs_query.h"

using namespace xs;

namespace {

// ---- MLST typing: every locus of a scheme, rows reduced on the device -----------
// The reads are in HBM once (uploaded into the first locus' buffers, or a device reader's batch).
// They are probed in chunks of R reads, R x Dmax x 4 <= the workspace: per chunk and locus the
// probe fills the rows buffer and mlst_top_kernel reduces it into column l of the n x loci device
// outputs, so the rows buffer does not grow with n and no hit matrix crosses PCIe.  Everything
// runs on the first locus' stream; its buffers hold the reads, the rows and the outputs.
constexpr uint64_t kMlstTypeWs = 4ull << 30;  // default cap of the rows buffer
constexpr size_t kTypeRingMin = 1u << 20;     // outputs of this size and more cross through the D2H ring
constexpr size_t kDirectRingMin = 64u << 20;  // xs_mlst_query's direct rows

struct MlstTypeOut {
    uint32_t *top, *top_score, *n_tied;  // n x loci each, host (n_tied may be null)
    uint64_t* num_kmers;                 // n, host (may be null)
    uint32_t n_ranks = 0;                // > 0: the ranked call (xs_mlst_type_ranked)
    uint32_t *rank_allele = nullptr, *rank_score = nullptr;  // n x loci x n_ranks each, host
};
static_assert(kMlstMaxRanks == XS_MLST_MAX_RANKS, "the kernels' cap and the header's");

// Where a span's ranks go on the device: rank j of (record r, locus l) at [(r * loci + l) * N + j].  N == 0: no ranks.
struct RankBufs {
    uint32_t N = 0;
    uint32_t *allele = nullptr, *score = nullptr;
    RankBufs at(uint64_t cell) const { return N ? RankBufs{N, allele + cell * N, score + cell * N} : RankBufs{}; }
};

// The argument errors of xs_mlst_type / xs_mlst_type_device that need no device.
int mlst_type_check(xs_bank* const* loci, uint32_t n_loci, uint64_t n, uint32_t step, const MlstTypeOut& out) {
    if (!loci || (n && (!out.top || !out.top_score))) return fail(XS_ERR_ARG, "null argument");
    if (n_loci == 0) return fail(XS_ERR_ARG, "n_loci must be >= 1");
    if (step == 0) return fail(XS_ERR_ARG, "step must be >= 1");
    for (uint32_t l = 0; l < n_loci; ++l) {
        if (!loci[l]) return fail(XS_ERR_ARG, "null argument");
        for (uint32_t j = 0; j < l; ++j)
            if (loci[j] == loci[l]) return fail(XS_ERR_ARG, "locus %u is the same handle as locus %u", l, j);
    }
    for (uint32_t l = 0; l < n_loci; ++l) {
        if (loci[l]->kind == XS_BANK_RBLOOM) return fail(XS_ERR_ARG, "MLST queries need a COBS bank (locus %u)", l);
        if (loci[l]->device != loci[0]->device) return fail(XS_ERR_ARG, "locus %u is on another device than locus 0", l);
        if (loci[l]->k != loci[0]->k) return fail(XS_ERR_ARG, "locus %u has another k than locus 0", l);
    }
    return XS_OK;
}

// The ranked calls' own argument errors.
int mlst_ranks_check(uint64_t n, const MlstTypeOut& out) {
    if (out.n_ranks == 0 || out.n_ranks > kMlstMaxRanks)
        return fail(XS_ERR_ARG, "n_ranks must be in 1 .. %u", kMlstMaxRanks);
    if (n && (!out.rank_allele || !out.rank_score)) return fail(XS_ERR_ARG, "null argument (rank outputs)");
    return XS_OK;
}

// The argument errors of xs_mlst_type_contigs / _device that need no device, then those that need the loci's k.
int mlst_contigs_check(xs_bank* const* loci, uint32_t n_loci, const uint64_t* width, const xs_mlst_chunk_rule_t* rule_in,
                       uint64_t seq_bytes, uint64_t n, uint32_t step, const MlstTypeOut& out,
                       xs_mlst_chunk_rule_t* rule) {
    if (!width) return fail(XS_ERR_ARG, "null argument (locus_width)");
    if (int rc = chunk_rule_check(rule_in, rule)) return rc;
    if (seq_bytes >= (1ull << 32) - 64)
        return fail(XS_ERR_ARG, "at most 2^32-65 sequence bytes per call (a summed score must fit uint32)");
    if (int rc = mlst_type_check(loci, n_loci, n, step, out)) return rc;
    const uint32_t k = loci[0]->k;
    for (uint32_t l = 0; l < n_loci; ++l)
        if (width[l] < k)
            return fail(XS_ERR_ARG, "locus_width[%u] = %llu is below k = %u", l, (unsigned long long)width[l], k);
    if (rule->long_len < k) return fail(XS_ERR_ARG, "long_len must be >= k = %u", k);
    return XS_OK;
}

// A typing call once its arguments are checked: every locus' mutex held, taken in address order (two
// calls over the same handles in any order cannot deadlock), and the first locus' device current.
// Once drain.s is set, the stream drains on exit, before the locks go.
struct TypeCall {
    std::vector<std::unique_lock<std::mutex>> held;
    DrainStream drain;
    int lock(xs_bank* const* loci, uint32_t n_loci) {
        std::vector<xs_bank*> order(loci, loci + n_loci);
        std::sort(order.begin(), order.end(), std::less<xs_bank*>());
        for (xs_bank* b : order) held.emplace_back(b->mu);
        HIPCHK(hipSetDevice(loci[0]->device));
        return XS_OK;
    }
    // host reads: into the first locus' buffers
    int upload(xs_bank* b0, const char* seqs, const uint64_t* offsets, uint64_t n, Inputs* in) {
        drain.s = b0->stream;
        if (int rc = ws_enter(b0, b0->stream)) return rc;
        return upload_reads(b0, seqs, offsets, n, b0->stream, in);
    }
};

// The device outputs of a typing call, in the first locus' buffers: the rows one probe fills (row_cap
// rows of the widest locus within the workspace), top / score / tied (n x loci each) and, when the
// caller wants them, the reads' k-mer counts; a ranked call's ranks (n x loci x N twice) in mc_ranks.
struct TypeBufs {
    uint64_t n, L, dmax = 1, ws, row_cap;
    uint32_t *rows = nullptr, *top = nullptr, *score = nullptr, *tied = nullptr;
    uint64_t* nk = nullptr;
    RankBufs ranks;
    TypeBufs(xs_bank* const* loci, uint32_t n_loci, uint64_t n_, uint64_t workspace_bytes)
        : n(n_), L(n_loci), ws(workspace_bytes ? workspace_bytes : kMlstTypeWs) {
        for (uint32_t l = 0; l < n_loci; ++l) dmax = std::max(dmax, loci[l]->D);
        row_cap = std::min<uint64_t>(std::max<uint64_t>(1, ws / (dmax * 4)), (1ull << 31) - 1);
    }
    int reserve(xs_bank* b0, uint64_t n_rows, const MlstTypeOut& out) {
        if (int rc = b0->hits.ensure(n_rows * dmax * 4)) return rc;
        if (int rc = b0->best.ensure(n * L * 4 * 3)) return rc;
        if (int rc = out.num_kmers ? b0->nk.ensure(n * 8) : XS_OK) return rc;
        rows = b0->hits.as<uint32_t>();
        top = b0->best.as<uint32_t>();
        score = top + n * L;
        tied = out.n_tied ? score + n * L : nullptr;
        nk = out.num_kmers ? b0->nk.as<uint64_t>() : nullptr;
        if (out.n_ranks) {
            const uint64_t cells = n * L * out.n_ranks;
            if (int rc = b0->mc_ranks.ensure(cells * 4 * 2)) return rc;
            ranks = RankBufs{out.n_ranks, b0->mc_ranks.as<uint32_t>(), b0->mc_ranks.as<uint32_t>() + cells};
        }
        return XS_OK;
    }
    int to_host(xs_bank* b0, const MlstTypeOut& out, hipStream_t s) const {
        const size_t rank_bytes = n * L * ranks.N * 4;
        const D2hPart parts[6] = {{out.top, top, n * L * 4},
                                  {out.top_score, score, n * L * 4},
                                  {out.n_tied, tied, tied ? n * L * 4 : 0},
                                  {out.num_kmers, nk, nk ? n * 8 : 0},
                                  {out.rank_allele, ranks.allele, rank_bytes},
                                  {out.rank_score, ranks.score, rank_bytes}};
        return d2h_parts(b0, parts, 6, kTypeRingMin, s);
    }
};

// n reads [r0, r0 + n) probed against every locus in pieces of `per` reads, each piece's rows reduced into
// columns of the outputs whose row 0 is the first read's (top / score / tied, and nk when wanted, point at
// it).  ho: the reads' offsets on the host ([0] = 0), or null: a piece's plans then take the batch's
// bytes, an upper bound, for its own.  The first locus' probe computes the k-mer counts.  ranks (its
// pointers at the first read's too): the ranked row kernel reduces each piece in place of the top kernel.
int mlst_type_span(xs_bank* const* loci, uint32_t n_loci, const Inputs& all, const uint64_t* ho, uint64_t r0, uint64_t n,
                   uint64_t per, uint32_t step, uint32_t* d_rows, uint32_t* top, uint32_t* score, uint32_t* tied,
                   uint64_t* nk, const RankBufs& ranks, hipStream_t s) {
    const uint64_t L = n_loci;
    for (uint64_t a = 0; a < n; a += per) {
        const uint64_t cn = std::min(per, n - a);
        const Inputs in{all.seqs, all.seq_bytes, all.offs + r0 + a, cn, ho ? ho[r0 + a + cn] - ho[r0 + a] : 0};
        for (uint32_t l = 0; l < n_loci; ++l) {
            if (int rc = run_query(loci[l], in, step, d_rows, l == 0 && nk ? nk + a : nullptr, nullptr, s)) return rc;
            const uint64_t o = a * L + l;
            if (ranks.N) {
                const RankBufs rk = ranks.at(o);
                HIPCHK(launch_mlst_ranks(d_rows, cn, loci[l]->D, rk.N, top + o, score + o, tied ? tied + o : nullptr, L,
                                         rk.allele, rk.score, L * rk.N, s));
            } else {
                HIPCHK(launch_mlst_top(d_rows, cn, loci[l]->D, top + o, score + o, tied ? tied + o : nullptr, L, s));
            }
        }
    }
    return XS_OK;
}

// The chunks, probes and reductions of one call, enqueued on the first locus' stream; then the
// outputs' copies to the host.  host_offs: the reads' offsets on the host (n + 1, [0] = 0) or null.
int mlst_type_run(xs_bank* const* loci, uint32_t n_loci, const Inputs& all, const uint64_t* host_offs, uint32_t step,
                  uint64_t workspace_bytes, const MlstTypeOut& out) {
    xs_bank* b0 = loci[0];
    const hipStream_t s = b0->stream;
    TypeBufs o(loci, n_loci, all.n, workspace_bytes);
    const uint64_t per = std::min(o.row_cap, all.n);
    if (int rc = ws_enter(b0, s)) return rc;
    if (int rc = o.reserve(b0, per, out)) return rc;
    if (int rc = mlst_type_span(loci, n_loci, all, host_offs, 0, o.n, per, step, o.rows, o.top, o.score, o.tied, o.nk,
                                RankBufs{}, s))
        return rc;
    if (int rc = ws_leave(b0, s)) return rc;
    return o.to_host(b0, out, s);
}

// ---- MLST typing of contigs: chunked, probed, summed and reduced on the device ----
// Records of long_len bytes and more follow the reference's chunk rule (xspect_hip.h), the others
// mlst_type_run's.  Short records are probed where they lie, run by run of consecutive records (or,
// when a batch interleaves so many runs that their launches would dominate, compacted once by
// gather_reads_kernel and their outputs scattered back).  Per locus the long records' chunks are
// numbered through and processed in ranges of at most R chunks (R rows of the widest locus within
// the workspace) and about as many text bytes: the splitter writes the range's chunk texts, the
// probe its rows, one pass adds them to the per-record accumulators and a wave per finished record
// writes its call.  A record cut by a range end keeps its accumulators in slot 0 of the next range.
// The host's part is the chunk runs, closed forms of the lengths: O(long records + ranges) per locus
// (xs_mlst_plan.h).
constexpr size_t kMaxShortRuns = 64;  // more runs of short records than this: compact them first

// What one contig call works on: the loci, the reads and their host offsets, and the stream.
struct ContigCall {
    xs_bank* const* loci;
    uint32_t n_loci;
    const Inputs& all;
    const uint64_t* ho;
    uint32_t step;
    hipStream_t s;
};

// Every locus' ranges and runs (one array, sent once), and the largest range's needs.
struct ContigPlan {
    std::vector<MlstChunkRun> runs;
    std::vector<ChunkRange> ranges;
    std::vector<size_t> locus_end;
    uint64_t max_nc = 0, max_bytes = 0, max_runs = 0;
};

// Short records where they lie: one span per run.
int type_short_in_place(const ContigCall& c, const RecordKinds& kinds, const TypeBufs& o) {
    for (const auto& run : kinds.short_runs) {
        const uint64_t at = run.first * o.L;
        if (int rc = mlst_type_span(c.loci, c.n_loci, c.all, c.ho, run.first, run.second - run.first, o.row_cap, c.step,
                                    o.rows, o.top + at, o.score + at, o.tied ? o.tied + at : nullptr, nullptr,
                                    o.ranks.at(at), c.s))
            return rc;
    }
    return XS_OK;
}

// Short records gathered into one batch of their own, typed as one span, their outputs scattered back.
int type_short_compacted(const ContigCall& c, const RecordKinds& kinds, const TypeBufs& o) {
    xs_bank* b0 = c.loci[0];
    const hipStream_t s = c.s;
    const uint64_t m = kinds.n_short, L = o.L, N = o.ranks.N;
    if (m >= (1ull << 32)) return fail(XS_ERR_ARG, "at most 2^32-1 short records per call");
    if (int rc = b0->mc_idx_h.ensure((m + 1) * 8 + m * 4)) return rc;
    if (int rc = b0->mc_idx.ensure((m + 1) * 8 + m * 4)) return rc;
    if (int rc = b0->mc_short.ensure(kinds.short_bytes + kPad)) return rc;
    if (int rc = b0->mc_out.ensure(m * L * 4 * (3 + 2 * N))) return rc;
    uint64_t* co = static_cast<uint64_t*>(b0->mc_idx_h.p);  // the compacted reads' m + 1 offsets, then their indices
    uint32_t* ci = reinterpret_cast<uint32_t*>(co + m + 1);
    uint64_t j = 0, ob = 0;
    for (const auto& run : kinds.short_runs)
        for (uint64_t r = run.first; r < run.second; ++r, ++j) {
            co[j] = ob;
            ci[j] = (uint32_t)r;
            ob += c.ho[r + 1] - c.ho[r];
        }
    co[m] = ob;
    HIPCHK(hipMemcpyAsync(b0->mc_idx.p, co, (m + 1) * 8 + m * 4, hipMemcpyHostToDevice, s));
    const uint64_t* d_co = b0->mc_idx.as<uint64_t>();
    const uint32_t* d_ci = reinterpret_cast<const uint32_t*>(d_co + m + 1);
    HIPCHK(launch_gather_reads(c.all.seqs, c.all.offs, d_ci, m, b0->mc_short.as<uint8_t>(), d_co, s));
    HIPCHK(hipMemsetAsync(b0->mc_short.as<uint8_t>() + kinds.short_bytes, 0, kPad, s));
    uint32_t* c_top = b0->mc_out.as<uint32_t>();
    uint32_t* c_score = c_top + m * L;
    uint32_t* c_tied = o.tied ? c_score + m * L : nullptr;
    const RankBufs c_ranks = N ? RankBufs{o.ranks.N, c_top + 3 * m * L, c_top + (3 + N) * m * L} : RankBufs{};
    const Inputs shorts{b0->mc_short.as<uint8_t>(), kinds.short_bytes, d_co, m};
    if (int rc = mlst_type_span(c.loci, c.n_loci, shorts, co, 0, m, o.row_cap, c.step, o.rows, c_top, c_score, c_tied,
                                nullptr, c_ranks, s))
        return rc;
    HIPCHK(launch_mlst_scatter_rows(d_ci, m, L, c_top, c_score, c_tied, o.top, o.score, o.tied, s));
    if (N)
        HIPCHK(launch_mlst_scatter_rows(d_ci, m, L * N, c_ranks.allele, c_ranks.score, nullptr, o.ranks.allele,
                                        o.ranks.score, nullptr, s));
    return XS_OK;
}

// Long records: locus by locus, range by range.
int type_long_ranges(const ContigCall& c, const ContigPlan& plan, uint32_t threshold, const TypeBufs& o) {
    xs_bank* b0 = c.loci[0];
    const hipStream_t s = c.s;
    const size_t run_bytes = plan.runs.size() * sizeof(MlstChunkRun);
    if (int rc = b0->mc_runs_h.ensure(run_bytes)) return rc;
    if (int rc = b0->mc_runs.ensure(run_bytes)) return rc;
    if (int rc = b0->mc_text.ensure(plan.max_bytes + kPad)) return rc;
    if (int rc = b0->mc_offs.ensure((plan.max_nc + 1) * 8)) return rc;
    if (int rc = b0->mc_sum.ensure(plan.max_runs * o.dmax * 8)) return rc;
    if (int rc = b0->mc_key.ensure(plan.max_runs * o.dmax * 8)) return rc;
    memcpy(b0->mc_runs_h.p, plan.runs.data(), run_bytes);
    HIPCHK(hipMemcpyAsync(b0->mc_runs.p, b0->mc_runs_h.p, run_bytes, hipMemcpyHostToDevice, s));
    uint8_t* text = b0->mc_text.as<uint8_t>();
    uint64_t* coffs = b0->mc_offs.as<uint64_t>();
    auto* sum = b0->mc_sum.as<unsigned long long>();
    auto* key = b0->mc_key.as<unsigned long long>();
    size_t gi = 0;
    for (uint32_t l = 0; l < c.n_loci; ++l) {
        const uint64_t D = c.loci[l]->D;
        for (; gi < plan.locus_end[l]; ++gi) {
            const ChunkRange& g = plan.ranges[gi];
            const MlstChunkRun* d_runs = b0->mc_runs.as<MlstChunkRun>() + g.run0;
            const uint64_t keep = g.carry_in ? 1 : 0;  // slot 0 holds the record the last range left unfinished
            if (g.n_runs > keep) {
                HIPCHK(hipMemsetAsync(sum + keep * D, 0, (g.n_runs - keep) * D * 8, s));
                HIPCHK(hipMemsetAsync(key + keep * D, 0xFF, (g.n_runs - keep) * D * 8, s));
            }
            HIPCHK(launch_mlst_split(c.all.seqs, d_runs, g.n_runs, g.nc, b0->k, text, coffs, s));
            const Inputs in{text, g.bytes, coffs, g.nc, g.bytes};
            if (int rc = run_query(c.loci[l], in, c.step, o.rows, nullptr, nullptr, s)) return rc;
            HIPCHK(launch_mlst_chunk_acc(o.rows, g.nc, D, &d_runs->row0, kMlstRunWords, g.n_runs, threshold, g.chunk_base,
                                         sum, key, s));
            const uint64_t done = g.n_runs - (g.carry_out ? 1 : 0);
            HIPCHK(launch_mlst_owner_top(sum, key, done, D, &d_runs->rec, kMlstRunWords, o.top + l, o.score + l,
                                         o.tied ? o.tied + l : nullptr, o.L, s));
            if (o.ranks.N) {
                const RankBufs rk = o.ranks.at(l);
                HIPCHK(launch_mlst_owner_ranks(sum, key, done, D, &d_runs->rec, kMlstRunWords, rk.N, rk.allele, rk.score,
                                               o.L * rk.N, s));
            }
            if (g.carry_out && done > 0) {
                HIPCHK(hipMemcpyAsync(sum, sum + done * D, D * 8, hipMemcpyDeviceToDevice, s));
                HIPCHK(hipMemcpyAsync(key, key + done * D, D * 8, hipMemcpyDeviceToDevice, s));
            }
        }
    }
    return XS_OK;
}

int mlst_contigs_run(xs_bank* const* loci, uint32_t n_loci, const uint64_t* width, const xs_mlst_chunk_rule_t& rule,
                     const Inputs& all, const uint64_t* ho, uint32_t step, uint64_t workspace_bytes,
                     const MlstTypeOut& out) {
    xs_bank* b0 = loci[0];
    const ContigCall c{loci, n_loci, all, ho, step, b0->stream};
    const uint64_t n = all.n;
    TypeBufs o(loci, n_loci, n, workspace_bytes);

    // classify and cut
    const RecordKinds kinds = classify_records(ho, n, rule.long_len);
    ContigPlan plan;
    for (uint32_t l = 0; l < n_loci; ++l) {
        cut_chunk_ranges(kinds.longs, ho, width[l], b0->k, rule, o.row_cap, std::max<uint64_t>(o.ws, 1), &plan.runs,
                         &plan.ranges);
        plan.locus_end.push_back(plan.ranges.size());
    }
    for (const ChunkRange& g : plan.ranges) {
        plan.max_nc = std::max(plan.max_nc, g.nc);
        plan.max_bytes = std::max(plan.max_bytes, g.bytes);
        plan.max_runs = std::max(plan.max_runs, g.n_runs);
    }

    // reserve
    if (int rc = ws_enter(b0, c.s)) return rc;
    const uint64_t short_per = std::min(o.row_cap, std::max<uint64_t>(kinds.n_short, 1));
    if (int rc = o.reserve(b0, std::max(short_per, plan.max_nc), out)) return rc;
    if (o.nk) {  // of every record, long ones too, from the lengths alone
        if (int rc = b0->nseg.ensure((n + 1) * 8)) return rc;
        HIPCHK(launch_units(all.offs, n, b0->k, step, o.nk, b0->nseg.as<uint64_t>(), c.s));
    }

    const bool compact = kinds.short_runs.size() > kMaxShortRuns;
    if (int rc = compact ? type_short_compacted(c, kinds, o) : type_short_in_place(c, kinds, o)) return rc;
    if (!plan.ranges.empty())
        if (int rc = type_long_ranges(c, plan, rule.threshold, o)) return rc;
    if (int rc = ws_leave(b0, c.s)) return rc;
    return o.to_host(b0, out, c.s);
}

// The (sum, key) accumulators of the chunk reductions alone (xs_mlst_chunk_top_device, xs_mlst_chunk_ranks_device):
// they live for the call only, which returns once its outputs are written.
struct OwnerAcc {
    DevBuf buf;
    unsigned long long *sum = nullptr, *key = nullptr;
    int fill(const uint32_t* d_hits, uint64_t n_chunks, uint64_t D, const uint64_t* d_owner_begin, uint64_t n_owners,
             uint32_t threshold, hipStream_t s) {
        const uint64_t cells = n_owners * D;
        if (int rc = buf.ensure(cells * 16)) return rc;
        sum = buf.as<unsigned long long>();
        key = sum + cells;
        HIPCHK(hipMemsetAsync(sum, 0, cells * 8, s));
        HIPCHK(hipMemsetAsync(key, 0xFF, cells * 8, s));
        HIPCHK(launch_mlst_chunk_acc(d_hits, n_chunks, D, d_owner_begin, 1, n_owners, threshold, 0, sum, key, s));
        return XS_OK;
    }
};

// xs_mlst_type_contigs and xs_mlst_type_ranked, from host reads.
int contigs_host(xs_bank* const* loci, uint32_t n_loci, const uint64_t* locus_width, const xs_mlst_chunk_rule_t* rule,
                 const char* seqs, const uint64_t* offsets, uint64_t n, uint32_t step, uint64_t workspace_bytes,
                 const MlstTypeOut& out) {
    if (!offsets || (!seqs && n)) return fail(XS_ERR_ARG, "null argument");
    xs_mlst_chunk_rule_t r;
    if (int rc = mlst_contigs_check(loci, n_loci, locus_width, rule, offsets[n] - offsets[0], n, step, out, &r)) return rc;
    TypeCall call;
    if (int rc = call.lock(loci, n_loci)) return rc;
    if (n == 0) return XS_OK;
    Inputs in;
    if (int rc = call.upload(loci[0], seqs, offsets, n, &in)) return rc;
    return mlst_contigs_run(loci, n_loci, locus_width, r, in, static_cast<const uint64_t*>(loci[0]->offs_h.p), step,
                            workspace_bytes, out);
}

// The same from reads already in HBM.
int contigs_device(xs_bank* const* loci, uint32_t n_loci, const uint64_t* locus_width, const xs_mlst_chunk_rule_t* rule,
                   const void* d_seqs, uint64_t seq_bytes, const uint64_t* d_offsets, const uint64_t* host_offsets,
                   uint64_t n, uint32_t step, uint64_t workspace_bytes, const MlstTypeOut& out) {
    if (n && (!d_seqs || !d_offsets)) return fail(XS_ERR_ARG, "null argument");
    xs_mlst_chunk_rule_t r;
    if (int rc = mlst_contigs_check(loci, n_loci, locus_width, rule, seq_bytes, n, step, out, &r)) return rc;
    TypeCall call;
    if (int rc = call.lock(loci, n_loci)) return rc;
    if (n == 0) return XS_OK;
    call.drain.s = loci[0]->stream;
    std::vector<uint64_t> copied;
    if (!host_offsets) {  // the lengths decide the chunk geometry: one copy back
        copied.resize(n + 1);
        HIPCHK(hipMemcpy(copied.data(), d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost));
        host_offsets = copied.data();
    }
    for (uint64_t i = 0; i < n; ++i)
        if (host_offsets[i + 1] < host_offsets[i]) return bad_offsets();
    if (host_offsets[0] != 0 || host_offsets[n] > seq_bytes)
        return fail(XS_ERR_ARG, "offsets must start at 0 and end within seq_bytes");
    const Inputs in{static_cast<const uint8_t*>(d_seqs), seq_bytes, d_offsets, n};
    return mlst_contigs_run(loci, n_loci, locus_width, r, in, host_offsets, step, workspace_bytes, out);
}

}  // namespace

extern "C" {

int xs_mlst_sum(xs_bank* b, const uint32_t* hits, const uint32_t* seq_of_chunk, uint64_t n_chunks,
                uint64_t n_seqs, uint32_t threshold, uint64_t* scores) {
    return xs::guard([&]() -> int {
        if (!b || (!hits && n_chunks) || (!seq_of_chunk && n_chunks) || !scores)
            return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(b->mu);
        HIPCHK(hipSetDevice(b->device));
        const uint64_t D = b->D;
        for (uint64_t c = 0; c < n_chunks; ++c)
            if (seq_of_chunk[c] >= n_seqs) return fail(XS_ERR_ARG, "seq_of_chunk[%llu] out of range", (unsigned long long)c);
        if (n_seqs == 0) return XS_OK;
        if (int rc = ws_enter(b, b->stream)) return rc;
        if (int rc = b->hits.ensure(n_chunks * D * 4 + 4)) return rc;
        if (int rc = b->tmp.ensure(n_chunks * 4 + 4)) return rc;
        if (int rc = b->totals.ensure(n_seqs * D * 8)) return rc;
        if (n_chunks) {
            HIPCHK(hipMemcpyAsync(b->hits.p, hits, n_chunks * D * 4, hipMemcpyHostToDevice, b->stream));
            HIPCHK(hipMemcpyAsync(b->tmp.p, seq_of_chunk, n_chunks * 4, hipMemcpyHostToDevice, b->stream));
        }
        HIPCHK(hipMemsetAsync(b->totals.p, 0, n_seqs * D * 8, b->stream));
        HIPCHK(launch_mlst_sum(b->hits.as<uint32_t>(), b->tmp.as<uint32_t>(), n_chunks, D, threshold,
                               b->totals.as<unsigned long long>(), nullptr, nullptr, b->stream));
        HIPCHK(hipMemcpyAsync(scores, b->totals.p, n_seqs * D * 8, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        return XS_OK;
    });
}

int xs_mlst_query(xs_bank* b, const char* seqs, const uint64_t* offsets, uint64_t n_direct, uint64_t n_chunks,
                  const uint32_t* chunk_owner, uint64_t n_owners, uint32_t step, uint32_t threshold,
                  uint32_t* direct_hits, uint64_t* owner_scores, uint32_t* owner_first,
                  uint32_t* owner_first_score) {
    return xs::guard([&]() -> int {
        const uint64_t n = n_direct + n_chunks;
        if (!b || !offsets || (!seqs && n) || (n_chunks && !chunk_owner)) return fail(XS_ERR_ARG, "null argument");
        if (b->kind == XS_BANK_RBLOOM) return fail(XS_ERR_ARG, "MLST queries need a COBS bank");
        if (owner_first_score && !owner_first) return fail(XS_ERR_ARG, "owner_first_score needs owner_first");
        for (uint64_t c = 0; c < n_chunks; ++c)
            if (chunk_owner[c] >= n_owners || (c && chunk_owner[c] < chunk_owner[c - 1]))
                return fail(XS_ERR_ARG, "chunk_owner must be non-decreasing and < n_owners (chunk %llu)",
                            (unsigned long long)c);
        if (n_chunks >= (1ull << 32) - 1) return fail(XS_ERR_ARG, "at most 2^32-2 chunks per call");
        std::lock_guard<std::mutex> lk(b->mu);
        HIPCHK(hipSetDevice(b->device));
        const uint64_t D = b->D, od = n_owners * D;
        if (n_owners) {
            if (owner_scores) memset(owner_scores, 0, od * 8);
            if (owner_first) memset(owner_first, 0xFF, od * 4);
            if (owner_first_score) memset(owner_first_score, 0, od * 4);
        }
        if (n == 0) return XS_OK;
        if (int rc = ws_enter(b, b->stream)) return rc;
        if (int rc = b->hits.ensure(n * D * 4)) return rc;
        uint32_t* d_hits = b->hits.as<uint32_t>();
        // every record probed in one pass; only the direct rows cross to the host
        HostQuery q{seqs, offsets, nullptr, n, step};
        q.d_hits = d_hits;
        if (int rc = query_host(b, q)) return rc;
        if (n_direct && direct_hits) {
            const D2hPart rows{direct_hits, d_hits, n_direct * D * 4};
            if (int rc = d2h_parts(b, &rows, 1, kDirectRingMin, b->stream)) return rc;
        }
        if (n_chunks && n_owners) {
            if (int rc = ws_enter(b, b->stream)) return rc;
            if (int rc = b->tmp.ensure(n_chunks * 4)) return rc;
            if (int rc = b->totals.ensure(od * 8)) return rc;
            if (int rc = b->best.ensure(od * 8)) return rc;
            uint32_t* d_first = b->best.as<uint32_t>();
            uint32_t* d_fscore = d_first + od;
            HIPCHK(hipMemcpyAsync(b->tmp.p, chunk_owner, n_chunks * 4, hipMemcpyHostToDevice, b->stream));
            HIPCHK(hipMemsetAsync(b->totals.p, 0, od * 8, b->stream));
            HIPCHK(hipMemsetAsync(d_first, 0xFF, od * 4, b->stream));
            HIPCHK(hipMemsetAsync(d_fscore, 0, od * 4, b->stream));
            HIPCHK(launch_mlst_sum(d_hits + n_direct * D, b->tmp.as<uint32_t>(), n_chunks, D, threshold,
                                   b->totals.as<unsigned long long>(), d_first, d_fscore, b->stream));
            if (owner_scores) HIPCHK(hipMemcpyAsync(owner_scores, b->totals.p, od * 8, hipMemcpyDeviceToHost, b->stream));
            if (owner_first) HIPCHK(hipMemcpyAsync(owner_first, d_first, od * 4, hipMemcpyDeviceToHost, b->stream));
            if (owner_first_score)
                HIPCHK(hipMemcpyAsync(owner_first_score, d_fscore, od * 4, hipMemcpyDeviceToHost, b->stream));
            if (int rc = ws_leave(b, b->stream)) return rc;
        }
        HIPCHK(hipStreamSynchronize(b->stream));
        return XS_OK;
    });
}

int xs_mlst_top_device(const uint32_t* d_hits, uint64_t n, uint64_t num_docs, uint32_t* d_top, uint32_t* d_top_score,
                       uint32_t* d_n_tied, uint64_t out_stride, void* stream) {
    return xs::guard([&]() -> int {
        if ((!d_hits || !d_top || !d_top_score) && n) return fail(XS_ERR_ARG, "null argument");
        if (num_docs == 0 || num_docs > 0xFFFFFFFFull) return fail(XS_ERR_ARG, "num_docs must be in 1 .. 2^32-1");
        if (out_stride == 0) return fail(XS_ERR_ARG, "out_stride must be >= 1");
        HIPCHK(launch_mlst_top(d_hits, n, num_docs, d_top, d_top_score, d_n_tied, out_stride,
                               static_cast<hipStream_t>(stream)));
        return XS_OK;
    });
}

int xs_mlst_type(xs_bank* const* loci, uint32_t n_loci, const char* seqs, const uint64_t* offsets, uint64_t n,
                 uint32_t step, uint64_t workspace_bytes, uint32_t* top, uint32_t* top_score, uint32_t* n_tied,
                 uint64_t* num_kmers_out) {
    return xs::guard([&]() -> int {
        const MlstTypeOut out{top, top_score, n_tied, num_kmers_out};
        if (!offsets || (!seqs && n)) return fail(XS_ERR_ARG, "null argument");
        if (int rc = mlst_type_check(loci, n_loci, n, step, out)) return rc;
        TypeCall call;
        if (int rc = call.lock(loci, n_loci)) return rc;
        if (n == 0) return XS_OK;
        Inputs in;
        if (int rc = call.upload(loci[0], seqs, offsets, n, &in)) return rc;
        return mlst_type_run(loci, n_loci, in, static_cast<const uint64_t*>(loci[0]->offs_h.p), step, workspace_bytes,
                             out);
    });
}

int xs_mlst_type_device(xs_bank* const* loci, uint32_t n_loci, const void* d_seqs, uint64_t seq_bytes,
                        const uint64_t* d_offsets, uint64_t n, uint32_t step, uint64_t workspace_bytes, uint32_t* top,
                        uint32_t* top_score, uint32_t* n_tied, uint64_t* num_kmers_out) {
    return xs::guard([&]() -> int {
        const MlstTypeOut out{top, top_score, n_tied, num_kmers_out};
        if (n && (!d_seqs || !d_offsets)) return fail(XS_ERR_ARG, "null argument");
        if (int rc = mlst_type_check(loci, n_loci, n, step, out)) return rc;
        TypeCall call;
        if (int rc = call.lock(loci, n_loci)) return rc;
        if (n == 0) return XS_OK;
        const Inputs in{static_cast<const uint8_t*>(d_seqs), seq_bytes, d_offsets, n};
        return mlst_type_run(loci, n_loci, in, nullptr, step, workspace_bytes, out);
    });
}

int xs_mlst_type_contigs(xs_bank* const* loci, uint32_t n_loci, const uint64_t* locus_width,
                         const xs_mlst_chunk_rule_t* rule, const char* seqs, const uint64_t* offsets, uint64_t n,
                         uint32_t step, uint64_t workspace_bytes, uint32_t* top, uint32_t* top_score, uint32_t* n_tied,
                         uint64_t* num_kmers_out) {
    return xs::guard([&]() -> int {
        const MlstTypeOut out{top, top_score, n_tied, num_kmers_out};
        return contigs_host(loci, n_loci, locus_width, rule, seqs, offsets, n, step, workspace_bytes, out);
    });
}

int xs_mlst_type_contigs_device(xs_bank* const* loci, uint32_t n_loci, const uint64_t* locus_width,
                                const xs_mlst_chunk_rule_t* rule, const void* d_seqs, uint64_t seq_bytes,
                                const uint64_t* d_offsets, const uint64_t* host_offsets, uint64_t n, uint32_t step,
                                uint64_t workspace_bytes, uint32_t* top, uint32_t* top_score, uint32_t* n_tied,
                                uint64_t* num_kmers_out) {
    return xs::guard([&]() -> int {
        const MlstTypeOut out{top, top_score, n_tied, num_kmers_out};
        return contigs_device(loci, n_loci, locus_width, rule, d_seqs, seq_bytes, d_offsets, host_offsets, n, step,
                              workspace_bytes, out);
    });
}

int xs_mlst_type_ranked(xs_bank* const* loci, uint32_t n_loci, const uint64_t* locus_width,
                        const xs_mlst_chunk_rule_t* rule, const char* seqs, const uint64_t* offsets, uint64_t n,
                        uint32_t step, uint64_t workspace_bytes, uint32_t n_ranks, uint32_t* top, uint32_t* top_score,
                        uint32_t* n_tied, uint64_t* num_kmers_out, uint32_t* rank_allele, uint32_t* rank_score) {
    return xs::guard([&]() -> int {
        const MlstTypeOut out{top, top_score, n_tied, num_kmers_out, n_ranks, rank_allele, rank_score};
        if (int rc = mlst_ranks_check(n, out)) return rc;
        return contigs_host(loci, n_loci, locus_width, rule, seqs, offsets, n, step, workspace_bytes, out);
    });
}

int xs_mlst_type_ranked_device(xs_bank* const* loci, uint32_t n_loci, const uint64_t* locus_width,
                               const xs_mlst_chunk_rule_t* rule, const void* d_seqs, uint64_t seq_bytes,
                               const uint64_t* d_offsets, const uint64_t* host_offsets, uint64_t n, uint32_t step,
                               uint64_t workspace_bytes, uint32_t n_ranks, uint32_t* top, uint32_t* top_score,
                               uint32_t* n_tied, uint64_t* num_kmers_out, uint32_t* rank_allele,
                               uint32_t* rank_score) {
    return xs::guard([&]() -> int {
        const MlstTypeOut out{top, top_score, n_tied, num_kmers_out, n_ranks, rank_allele, rank_score};
        if (int rc = mlst_ranks_check(n, out)) return rc;
        return contigs_device(loci, n_loci, locus_width, rule, d_seqs, seq_bytes, d_offsets, host_offsets, n, step,
                              workspace_bytes, out);
    });
}

int xs_mlst_split_size(const uint64_t* lengths, uint64_t n_long, uint64_t width, uint32_t k,
                       const xs_mlst_chunk_rule_t* rule, uint64_t* n_chunks, uint64_t* chunk_bytes) {
    return xs::guard([&]() -> int {
        if ((!lengths && n_long) || !n_chunks || !chunk_bytes) return fail(XS_ERR_ARG, "null argument");
        xs_mlst_chunk_rule_t r;
        if (int rc = split_args_check(rule, width, k, &r)) return rc;
        uint64_t c = 0, b = 0;
        for (uint64_t i = 0; i < n_long; ++i) {
            const MlstRecGeom g =
                mlst_rec_geom(lengths[i], mlst_chunk_width(lengths[i], width, r.scale10_len, r.scale100_len), k);
            c += g.chunks;
            b += g.bytes;
        }
        *n_chunks = c;
        *chunk_bytes = b;
        return XS_OK;
    });
}

int xs_mlst_split_device(const void* d_seqs, const uint64_t* d_offsets, const uint32_t* d_long_index, uint64_t n_long,
                         uint64_t width, uint32_t k, const xs_mlst_chunk_rule_t* rule, void* d_chunk_seqs,
                         uint64_t* d_chunk_offsets, uint64_t* d_owner_begin, void* stream) {
    return xs::guard([&]() -> int {
        if (!d_chunk_seqs || !d_chunk_offsets || !d_owner_begin || (n_long && (!d_seqs || !d_offsets || !d_long_index)))
            return fail(XS_ERR_ARG, "null argument");
        xs_mlst_chunk_rule_t r;
        if (int rc = split_args_check(rule, width, k, &r)) return rc;
        const hipStream_t s = static_cast<hipStream_t>(stream);
        // the runs live for this call only: it returns once the chunks are written
        DevBuf runs;
        if (int rc = runs.ensure((n_long + 1) * sizeof(MlstChunkRun))) return rc;
        HIPCHK(launch_mlst_runs(d_offsets, d_long_index, n_long, width, k, r.scale10_len, r.scale100_len,
                                runs.as<MlstChunkRun>(), d_owner_begin, s));
        uint64_t nc = 0;
        HIPCHK(hipMemcpyAsync(&nc, d_owner_begin + n_long, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(launch_mlst_split(static_cast<const uint8_t*>(d_seqs), runs.as<MlstChunkRun>(), n_long, nc, k,
                                 static_cast<uint8_t*>(d_chunk_seqs), d_chunk_offsets, s));
        HIPCHK(hipStreamSynchronize(s));
        return XS_OK;
    });
}

int xs_mlst_chunk_top_device(const uint32_t* d_hits, uint64_t n_chunks, uint64_t num_docs,
                             const uint64_t* d_owner_begin, uint64_t n_owners, uint32_t threshold, uint32_t* d_top,
                             uint32_t* d_top_score, uint32_t* d_n_tied, uint64_t out_stride, void* stream) {
    return xs::guard([&]() -> int {
        if ((n_owners && (!d_owner_begin || !d_top || !d_top_score)) || (n_chunks && !d_hits))
            return fail(XS_ERR_ARG, "null argument");
        if (num_docs == 0 || num_docs > 0xFFFFFFFFull) return fail(XS_ERR_ARG, "num_docs must be in 1 .. 2^32-1");
        if (out_stride == 0) return fail(XS_ERR_ARG, "out_stride must be >= 1");
        if (n_chunks >= (1ull << 32)) return fail(XS_ERR_ARG, "at most 2^32-1 chunks per call");
        if (n_owners == 0) return XS_OK;
        const hipStream_t s = static_cast<hipStream_t>(stream);
        OwnerAcc acc;
        if (int rc = acc.fill(d_hits, n_chunks, num_docs, d_owner_begin, n_owners, threshold, s)) return rc;
        HIPCHK(launch_mlst_owner_top(acc.sum, acc.key, n_owners, num_docs, nullptr, 0, d_top, d_top_score, d_n_tied,
                                     out_stride, s));
        HIPCHK(hipStreamSynchronize(s));
        return XS_OK;
    });
}

int xs_mlst_ranks_device(const uint32_t* d_hits, uint64_t n, uint64_t num_docs, uint32_t n_ranks, uint32_t* d_top,
                         uint32_t* d_top_score, uint32_t* d_n_tied, uint64_t top_stride, uint32_t* d_rank_allele,
                         uint32_t* d_rank_score, uint64_t rank_stride, void* stream) {
    return xs::guard([&]() -> int {
        if ((!d_hits || !d_rank_allele || !d_rank_score) && n) return fail(XS_ERR_ARG, "null argument");
        if (num_docs == 0 || num_docs > 0xFFFFFFFFull) return fail(XS_ERR_ARG, "num_docs must be in 1 .. 2^32-1");
        if (n_ranks == 0 || n_ranks > kMlstMaxRanks) return fail(XS_ERR_ARG, "n_ranks must be in 1 .. %u", kMlstMaxRanks);
        if (rank_stride < n_ranks) return fail(XS_ERR_ARG, "rank_stride must be >= n_ranks");
        if ((d_top || d_top_score || d_n_tied) && top_stride == 0) return fail(XS_ERR_ARG, "top_stride must be >= 1");
        HIPCHK(launch_mlst_ranks(d_hits, n, num_docs, n_ranks, d_top, d_top_score, d_n_tied, top_stride, d_rank_allele,
                                 d_rank_score, rank_stride, static_cast<hipStream_t>(stream)));
        return XS_OK;
    });
}

int xs_mlst_chunk_ranks_device(const uint32_t* d_hits, uint64_t n_chunks, uint64_t num_docs,
                               const uint64_t* d_owner_begin, uint64_t n_owners, uint32_t threshold, uint32_t n_ranks,
                               uint32_t* d_rank_allele, uint32_t* d_rank_score, uint64_t rank_stride, void* stream) {
    return xs::guard([&]() -> int {
        if ((n_owners && (!d_owner_begin || !d_rank_allele || !d_rank_score)) || (n_chunks && !d_hits))
            return fail(XS_ERR_ARG, "null argument");
        if (num_docs == 0 || num_docs > 0xFFFFFFFFull) return fail(XS_ERR_ARG, "num_docs must be in 1 .. 2^32-1");
        if (n_ranks == 0 || n_ranks > kMlstMaxRanks) return fail(XS_ERR_ARG, "n_ranks must be in 1 .. %u", kMlstMaxRanks);
        if (rank_stride < n_ranks) return fail(XS_ERR_ARG, "rank_stride must be >= n_ranks");
        if (n_chunks >= (1ull << 32)) return fail(XS_ERR_ARG, "at most 2^32-1 chunks per call");
        if (n_owners == 0) return XS_OK;
        const hipStream_t s = static_cast<hipStream_t>(stream);
        OwnerAcc acc;
        if (int rc = acc.fill(d_hits, n_chunks, num_docs, d_owner_begin, n_owners, threshold, s)) return rc;
        HIPCHK(launch_mlst_owner_ranks(acc.sum, acc.key, n_owners, num_docs, nullptr, 0, n_ranks, d_rank_allele,
                                       d_rank_score, rank_stride, s));
        HIPCHK(hipStreamSynchronize(s));
        return XS_OK;
    });
}

}  // extern "C"
