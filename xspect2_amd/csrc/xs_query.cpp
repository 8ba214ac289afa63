// xs_query.cpp — queries and builds on a bank handle: the probe dispatcher (run_query), the chunked
// host pipeline (query_host), the small-call path (query_small), the host <-> device copy helpers and
// the xs_bank_build* / xs_query* entry points.  What xs_mlst.cpp takes from here is in xs_query.h.
#include <memory>

#include "xs_hitsink.h"
#include "xs_query.h"

using namespace xs;

namespace {

// ---- query / build pipeline --------------------------------------------------
// The unit-map buffers of n reads of `bytes` bytes in all.  query_host reserves them for its whole
// batch up front, so that no chunk's prepare_units grows one (an implicit device sync) mid-batch.
int reserve_units(xs_bank* b, uint64_t n, uint64_t bytes) {
    if (int rc = b->nseg.ensure((n + 1) * 8)) return rc;
    if (int rc = b->unit_ofs.ensure((n + 1) * 8)) return rc;
    if (int rc = b->n_units.ensure(2 * sizeof(uint64_t))) return rc;
    if (int rc = b->unit_read.ensure((n + bytes / kSegKmers + 1) * 4)) return rc;
    return b->scan_tmp.ensure(scan_temp_bytes(n ? n : 1));
}

// Unit decomposition (k-mer counts, units, unit -> read map) for n device-resident reads.
// units = false (the partitioned COBS probe, which maps k-mers to reads itself and
// zeroes the hit matrix): only the per-read k-mer counts, when the caller wants them.
int prepare_units(xs_bank* b, const Inputs& in, uint32_t step, uint64_t* d_nk, uint32_t* hits_zero,
                  uint64_t zero_cols, hipStream_t s, ReadView* rv, bool units = true) {
    if (int rc = reserve_units(b, in.n, in.plan_bytes())) return rc;
    if (units || d_nk) HIPCHK(launch_units(in.offs, in.n, b->k, step, d_nk, b->nseg.as<uint64_t>(), s));
    if (units) {
        HIPCHK(launch_scan(b->scan_tmp.p, b->scan_tmp.cap, b->nseg.as<uint64_t>(),
                           b->unit_ofs.as<uint64_t>(), in.n, s));
        HIPCHK(launch_scatter_units(b->nseg.as<uint64_t>(), b->unit_ofs.as<uint64_t>(), in.n,
                                    b->unit_read.as<uint32_t>(), b->n_units.as<uint64_t>(), hits_zero,
                                    zero_cols, s));
    }
    *rv = ReadView{in.seqs, in.seq_bytes, in.offs, b->unit_read.as<uint32_t>(), b->unit_ofs.as<uint64_t>(),
                   b->n_units.as<uint64_t>(), in.n, b->k, step};
    return XS_OK;
}

int probe_grid(xs_bank* b) {
    HIPCHK(hipSetDevice(b->device));
    const int g = b->kind == XS_BANK_RBLOOM ? probe_grid_bloom() : probe_grid_cobs(b->cobs_view(), b->k);
    return g > 0 ? g : 1;
}

// rbloom: the previous query's totals (members, k-mers), once their copy has landed, steer the next path choice
void poll_member_frac(xs_bank* b) {
    const hipError_t q = b->bloom_pending ? hipEventQuery(b->bloom_ev) : hipErrorNotReady;
    (void)hipGetLastError();  // hipErrorNotReady is not an error here
    if (q != hipSuccess) return;
    const uint64_t* t = static_cast<const uint64_t*>(b->bloom_tot_h.p);
    if (t[1]) b->member_frac = (double)t[0] / (double)t[1];
    b->bloom_pending = false;
}

// The partitioned probes' workspace is transient: when HBM cannot hold it, the query takes
// the direct / gather probe instead of failing (false).  miss_bytes = 0 (COBS): no miss bitmap.
bool reserve_part_ws(xs_bank* b, const PartSizes& z) {
    if (b->pk_nkc.ensure(z.nkc_bytes) || b->pk_kofs.ensure(z.nkc_bytes) || b->pk_scan.ensure(z.scan_bytes) ||
        b->pk_entries.ensure(z.entry_bytes) || b->pk_tbl.ensure(z.tbl_bytes) ||
        (z.miss_bytes && b->pk_miss.ensure(z.miss_bytes)) || b->pk_aux.ensure(z.aux_bytes)) {
        (void)hipGetLastError();
        return false;
    }
    return true;
}

}  // namespace

int xs::run_query(xs_bank* b, const Inputs& in, uint32_t step, uint32_t* d_hits, uint64_t* d_nk,
                  uint64_t* d_totals, hipStream_t s) {
    if (step == 0) return fail(XS_ERR_ARG, "step must be >= 1");
    if (in.n >= (1ull << 31)) return fail(XS_ERR_ARG, "at most 2^31-1 reads per call");
    if (int rc = ws_enter(b, s)) return rc;
    const bool bloom = b->kind == XS_BANK_RBLOOM;
    // the COBS path is chosen first: the partitioned probe needs no unit map
    CobsPartPlan cplan;
    bool cobs_part = false;
    if (!bloom) {
        cobs_part = cobs_part_plan(b->cobs_view(), b->k, in.n, in.plan_bytes(), step, b->opt, &cplan) &&
                    reserve_part_ws(b, cplan);
        (void)hipGetLastError();  // an earlier call's failure left on this thread is not this query's (the launchers read it)
    }
    ReadView rv;
    if (int rc = prepare_units(b, in, step, d_nk, d_hits, b->cols(), s, &rv, !cobs_part)) return rc;
    const int blocks = probe_grid(b);
    uint64_t* partials = nullptr;
    const uint64_t pcols = b->cols() + 1;
    if (d_totals || bloom) {  // rbloom always: its totals steer the next query's path
        if (int rc = b->partials.ensure((size_t)blocks * pcols * 8)) return rc;
        partials = b->partials.as<uint64_t>();
    }
    if (bloom) poll_member_frac(b);
    // probe events: at most kPassMarksMax queries between two xs_bank_probe_stats
    const bool timed = b->profiling && b->events_used < kPassMarksMax;
    if (timed) {
        if (b->events_used == b->events.size()) {
            hipEvent_t a, c;
            HIPCHK(hipEventCreate(&a));
            HIPCHK(hipEventCreate(&c));
            b->events.emplace_back(a, c);
        }
        HIPCHK(hipEventRecord(b->events[b->events_used].first, s));
    }
    BloomPartPlan plan;
    int path = XS_PATH_GATHER;
    const char* kernel = "";
    const bool bloom_part = bloom &&
                            bloom_part_plan(b->bloom_view(), in.n, in.plan_bytes(), step, b->member_frac, b->opt, &plan) &&
                            reserve_part_ws(b, plan);
    if (bloom_part || cobs_part) {
        path = XS_PATH_PARTITIONED;
        kernel = bloom ? "bloompart" : "cobspart";
        // pk_miss is the rbloom plans' alone: null on a COBS bank
        const PartWs ws{b->pk_nkc.as<uint64_t>(), b->pk_kofs.as<uint64_t>(), b->pk_scan.p, b->pk_scan.cap,
                        b->pk_entries.p, b->pk_tbl.as<uint16_t>(), b->pk_miss.as<uint32_t>(),
                        b->pk_aux.as<uint32_t>()};
        PassRecorder rec{&b->pass_ev, &b->pass_tag, &b->pass_used};
        PassRecorder* prec = b->profiling ? &rec : nullptr;
        HIPCHK(bloom ? launch_probe_bloom_part(rv, b->bloom_view(), plan, ws, d_hits, partials, blocks, s, prec)
                     : launch_probe_cobs_part(rv, b->cobs_view(), cplan, ws, d_hits, partials, blocks, s, prec));
    } else if (bloom) {
        HIPCHK(launch_probe_bloom(rv, b->bloom_view(), d_hits, partials, blocks, s, &kernel));
    } else {
        HIPCHK(launch_probe_cobs(rv, b->cobs_view(), d_hits, partials, blocks, s, &kernel));
    }
    b->last_path = path;
    b->last_kernel = kernel;
    if (timed) {
        HIPCHK(hipEventRecord(b->events[b->events_used].second, s));
        ++b->events_used;
    }
    if (d_totals) HIPCHK(launch_reduce_partials(partials, blocks, pcols, d_totals, s));
    if (bloom && !b->bloom_pending) {
        if (int rc = b->bloom_tot.ensure(2 * sizeof(uint64_t))) return rc;
        if (int rc = b->bloom_tot_h.ensure(2 * sizeof(uint64_t))) return rc;
        if (!b->bloom_ev) HIPCHK(hipEventCreateWithFlags(&b->bloom_ev, hipEventDisableTiming));
        HIPCHK(launch_reduce_partials(partials, blocks, pcols, b->bloom_tot.as<uint64_t>(), s));
        HIPCHK(hipMemcpyAsync(b->bloom_tot_h.p, b->bloom_tot.p, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipEventRecord(b->bloom_ev, s));
        b->bloom_pending = true;
    }
    return ws_leave(b, s);
}

// ---- host <-> device copies ------------------------------------------------------
// A host batch's per-read passes run before its first copy, in the call's critical path: on
// one thread below kSerialReads reads.
constexpr uint64_t kSerialReads = 1u << 18;
constexpr size_t kHostChunk = 32u << 20;  // a slot of the H2D staging ring
constexpr size_t kHostFirst = 8u << 20;

bool xs::rebase_offsets(const uint64_t* offsets, uint64_t n, uint64_t* dst) {
    const uint64_t base = offsets[0];
    bool bad[8] = {};
    par_ranges(n, kSerialReads, host_threads(), [&](int t, uint64_t a, uint64_t e) {
        bool ok = true;
        for (uint64_t r = a; r < e; ++r) {
            ok &= offsets[r + 1] >= offsets[r];
            dst[r] = offsets[r] - base;
        }
        bad[t] = !ok;
    });
    dst[n] = offsets[n] - base;
    return std::none_of(bad, bad + 8, [](bool x) { return x; });
}
int xs::bad_offsets() { return fail(XS_ERR_ARG, "offsets must be non-decreasing"); }

int xs::upload_reads(xs_bank* b, const char* seqs, const uint64_t* offsets, uint64_t n, hipStream_t s, Inputs* in) {
    if (int rc = b->offs_h.ensure((n + 1) * 8)) return rc;
    uint64_t* rb = static_cast<uint64_t*>(b->offs_h.p);
    if (!rebase_offsets(offsets, n, rb)) return bad_offsets();
    const uint64_t bytes = rb[n];
    if (int rc = b->seqs.ensure(bytes + kPad)) return rc;
    if (int rc = b->offs.ensure((n + 1) * 8)) return rc;
    HIPCHK(hipMemcpyAsync(b->offs.p, rb, (n + 1) * 8, hipMemcpyHostToDevice, s));
    const char* src = seqs + offsets[0];
    if (bytes && (bytes <= kHostFirst || is_pinned_host(src))) {
        HIPCHK(hipMemcpyAsync(b->seqs.p, src, bytes, hipMemcpyHostToDevice, s));
    } else if (bytes) {
        for (int i = 0; i < 2; ++i) {
            if (int rc = b->hstage[i].ensure(kHostChunk)) return rc;
            if (!b->hstage_ev[i]) HIPCHK(hipEventCreateWithFlags(&b->hstage_ev[i], hipEventDisableTiming));
        }
        const int threads = host_threads();
        uint64_t i = 0;
        for (uint64_t off = 0; off < bytes; off += kHostChunk, ++i) {
            const int slot = (int)(i & 1);
            const size_t nb = (size_t)std::min<uint64_t>(kHostChunk, bytes - off);
            if (i >= 2) HIPCHK(hipEventSynchronize(b->hstage_ev[slot]));  // the slot's last H2D is done
            par_memcpy(b->hstage[slot].p, src + off, nb, threads);
            HIPCHK(hipMemcpyAsync(b->seqs.as<uint8_t>() + off, b->hstage[slot].p, nb, hipMemcpyHostToDevice, s));
            HIPCHK(hipEventRecord(b->hstage_ev[slot], s));
        }
    }
    *in = Inputs{b->seqs.as<uint8_t>(), bytes, b->offs.as<uint64_t>(), n};
    return XS_OK;
}

int xs::d2h_parts(xs_bank* b, const D2hPart* parts, int n_parts, size_t ring_min, hipStream_t st) {
    constexpr size_t kChunk = 32u << 20;
    const int threads = host_threads();
    char* prev_host = nullptr;
    size_t prev_n = 0, i = 0;
    int prev_slot = -1;
    for (int p = 0; p < n_parts; ++p) {
        const D2hPart& part = parts[p];
        if (!part.bytes) continue;
        if (part.bytes < ring_min || is_pinned_host(part.host)) {
            HIPCHK(hipMemcpyAsync(part.host, part.dev, part.bytes, hipMemcpyDeviceToHost, st));
            continue;
        }
        for (size_t off = 0; off < part.bytes; off += kChunk, ++i) {
            const int slot = (int)(i & 1);  // free: its piece i - 2 was copied out while piece i - 1 crossed
            const size_t nb = std::min(kChunk, part.bytes - off);
            if (int rc = b->stage[slot].ensure(kChunk)) return rc;
            if (!b->stage_ev[slot]) HIPCHK(hipEventCreateWithFlags(&b->stage_ev[slot], hipEventDisableTiming));
            HIPCHK(hipMemcpyAsync(b->stage[slot].p, static_cast<const char*>(part.dev) + off, nb,
                                  hipMemcpyDeviceToHost, st));
            HIPCHK(hipEventRecord(b->stage_ev[slot], st));
            if (prev_slot >= 0) {
                HIPCHK(hipEventSynchronize(b->stage_ev[prev_slot]));
                par_memcpy(prev_host, b->stage[prev_slot].p, prev_n, threads);
            }
            prev_host = static_cast<char*>(part.host) + off;
            prev_n = nb;
            prev_slot = slot;
        }
    }
    if (prev_slot >= 0) {
        HIPCHK(hipEventSynchronize(b->stage_ev[prev_slot]));
        par_memcpy(prev_host, b->stage[prev_slot].p, prev_n, threads);
    }
    HIPCHK(hipStreamSynchronize(st));
    return XS_OK;
}

namespace {

// ---- host batches: staging overlapped with the probe --------------------------
// A host batch is cut at read boundaries into chunks of about kHostChunk
// sequence bytes (the first smaller, so the probe starts early).  Chunk i is
// copied into a pinned slot by host threads and sent on the copy stream while
// the bank stream probes chunk i-1.  With host hits wanted, chunk i-1's hit
// rows go back through the D2H ring on a third stream while chunk i is probed
// (HitSink).  Device buffers span the whole batch, so chunks never overwrite
// each other's reads or hits, and the workspace is sized for the whole batch up
// front (no reallocation, hence no implicit device sync, between chunks).
constexpr uint64_t kDevChunkReads = 1u << 18;  // device reads: the smallest chunk, in reads

// The batch cut into chunks: chunk i is reads [cut[i], cut[i + 1]), whose bytes start at ofs[i]
// (offsets rebased to 0); `bytes` bounds the batch's last offset.
struct Chunks {
    std::vector<uint64_t> cut{0}, ofs;
    uint64_t bytes = 0;
    size_t count() const { return cut.size() - 1; }
};

// Phase 1, host reads: the offsets checked and rebased to 0 into pinned memory (their H2D copy
// then needs no staging), and cuts of about kHostChunk bytes.
int cut_host_chunks(xs_bank* b, const HostQuery& q, Chunks* c) {
    if (int rc = b->offs_h.ensure((q.n + 1) * 8)) return rc;
    uint64_t* rb = static_cast<uint64_t*>(b->offs_h.p);
    if (!rebase_offsets(q.offsets, q.n, rb)) return bad_offsets();
    for (size_t limit = kHostFirst; c->cut.back() < q.n; limit = kHostChunk) {
        const uint64_t r0 = c->cut.back();
        const uint64_t e = (uint64_t)(std::upper_bound(rb + r0 + 1, rb + q.n + 1, rb[r0] + limit) - rb) - 1;
        c->cut.push_back(e > r0 ? e : r0 + 1);  // a read over the limit is a chunk of its own
    }
    for (uint64_t r : c->cut) c->ofs.push_back(rb[r]);
    c->bytes = rb[q.n];
    return XS_OK;
}

// Phase 1, device reads: chunks overlap the hit rows' D2H with the next chunk's probe; without
// rows to bring back, one chunk (a partitioned probe reloads the bank's partitions into L2 per chunk).
int cut_dev_chunks(xs_bank* b, const HostQuery& q, Chunks* c) {
    const uint64_t per = q.hits_host ? std::max<uint64_t>(kDevChunkReads, (q.n + 3) / 4) : q.n;
    while (c->cut.back() < q.n) c->cut.push_back(std::min(q.n, c->cut.back() + per));
    c->bytes = q.dev->seq_bytes;
    if (c->cut.size() == 2) {
        // one chunk: its bytes are the batch's (offsets start at 0; seq_bytes bounds the
        // last offset, which is all the probe's planner needs), no round trip to the device
        c->ofs = {0, q.dev->seq_bytes};
        return XS_OK;
    }
    if (int rc = b->cut_ofs.ensure(c->cut.size() * 8)) return rc;
    for (size_t j = 0; j < c->cut.size(); ++j)
        HIPCHK(hipMemcpyAsync(static_cast<uint64_t*>(b->cut_ofs.p) + j, q.dev->offs + c->cut[j], 8,
                              hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    const uint64_t* o = static_cast<const uint64_t*>(b->cut_ofs.p);
    c->ofs.assign(o, o + c->cut.size());
    return XS_OK;
}

// Phase 2: the workspace for the whole batch, and the streams and events its chunks use.
int reserve_host_query(xs_bank* b, const HostQuery& q, const Chunks& c, int wire) {
    const uint64_t n = q.n, pcols = b->cols() + 1;
    if (!q.dev) {
        if (int rc = b->seqs.ensure(c.bytes + kPad)) return rc;
        if (int rc = b->offs.ensure((n + 1) * 8)) return rc;
    }
    if (int rc = reserve_units(b, n, c.bytes)) return rc;
    if (int rc = b->partials.ensure((size_t)probe_grid(b) * pcols * 8)) return rc;
    if (q.tot_host)
        if (int rc = b->totals.ensure(c.count() * pcols * 8)) return rc;
    if (!q.dev) {  // host reads: the H2D staging ring and its copy stream (device reads need neither)
        for (int s = 0; s < 2; ++s) {
            if (int rc = b->hstage[s].ensure(kHostChunk)) return rc;
            if (!b->hstage_ev[s]) HIPCHK(hipEventCreateWithFlags(&b->hstage_ev[s], hipEventDisableTiming));
        }
        if (!b->copy_stream) HIPCHK(hipStreamCreateWithFlags(&b->copy_stream, hipStreamNonBlocking));
    }
    if (q.hits_host && !b->d2h_stream) HIPCHK(hipStreamCreateWithFlags(&b->d2h_stream, hipStreamNonBlocking));
    if (q.hits_host && wire != 4) {
        if (int rc = b->narrow.ensure(n * b->cols() * (uint64_t)wire + 16)) return rc;
        if (int rc = b->ovf.ensure(sizeof(uint32_t))) return rc;
        HIPCHK(hipMemsetAsync(b->ovf.p, 0, sizeof(uint32_t), b->stream));
    }
    while (q.hits_host && b->chunk_ev.size() < c.count()) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        b->chunk_ev.push_back(e);
    }
    return XS_OK;
}

// Phase 3: chunk by chunk, stage the reads (host reads), probe, and hand the rows to the sink.
int run_chunks(xs_bank* b, const HostQuery& q, const Chunks& c, int wire) {
    const uint64_t n = q.n, cols = b->cols(), pcols = cols + 1;
    const size_t nc = c.count();
    const bool narrowing = q.hits_host && wire != 4;
    const uint8_t* d_seqs = q.dev ? q.dev->seqs : b->seqs.as<uint8_t>();
    const uint64_t* d_offs = q.dev ? q.dev->offs : b->offs.as<uint64_t>();
    // whatever way the call ends (an error return included), no H2D copy may still be
    // reading the caller's reads or the rebased offsets once it has: the copy stream drains on exit
    DrainStream drain;
    if (!q.dev) {
        drain.s = b->copy_stream;
        HIPCHK(hipMemcpyAsync(b->offs.p, b->offs_h.p, (n + 1) * 8, hipMemcpyHostToDevice, b->copy_stream));
    }
    const int threads = host_threads();
    // the hit rows go back behind the probe (HitSink: its own thread, stream and pinned ring)
    std::unique_ptr<HitSink> sink;
    if (q.hits_host) {
        sink.reset(new HitSink(b, q.hits_host, narrowing ? b->narrow.p : static_cast<const void*>(q.d_hits), cols, wire,
                               q.hit_bytes));
        if (int rc = sink->start(n * cols * (uint64_t)q.hit_bytes)) return rc;
    }
    bool used[2] = {false, false};
    for (size_t i = 0; i < nc; ++i) {
        const uint64_t r0 = c.cut[i], r1 = c.cut[i + 1], o0 = c.ofs[i], nb = c.ofs[i + 1] - o0;
        if (!q.dev) {
            const char* src = q.seqs + q.offsets[0] + o0;
            const int slot = (int)(i & 1);
            uint8_t* stage_dst = b->seqs.as<uint8_t>() + o0;
            if (used[slot]) HIPCHK(hipEventSynchronize(b->hstage_ev[slot]));  // the slot's last H2D is done
            if (nb && nb <= kHostChunk) {
                par_memcpy(b->hstage[slot].p, src, nb, threads);
                HIPCHK(hipMemcpyAsync(stage_dst, b->hstage[slot].p, nb, hipMemcpyHostToDevice, b->copy_stream));
            } else if (nb) {  // one read larger than a slot
                HIPCHK(hipMemcpyAsync(stage_dst, src, nb, hipMemcpyHostToDevice, b->copy_stream));
            }
            HIPCHK(hipEventRecord(b->hstage_ev[slot], b->copy_stream));
            used[slot] = true;
            HIPCHK(hipStreamWaitEvent(b->stream, b->hstage_ev[slot], 0));
        }
        const Inputs in{d_seqs, q.dev ? c.bytes : c.ofs[i + 1], d_offs + r0, r1 - r0, nb};
        if (int rc = run_query(b, in, q.step, q.d_hits ? q.d_hits + r0 * cols : nullptr, q.d_nk ? q.d_nk + r0 : nullptr,
                               q.tot_host ? b->totals.as<uint64_t>() + i * pcols : nullptr, b->stream))
            return rc;
        if (q.hits_host) {
            if (narrowing)
                HIPCHK(launch_narrow_hits(q.d_hits + r0 * cols, b->narrow.as<uint8_t>() + r0 * cols * wire,
                                          (r1 - r0) * cols, wire, b->stream, b->ovf.as<uint32_t>()));
            HIPCHK(hipEventRecord(b->chunk_ev[i], b->stream));
            sink->push(r0, r1, b->chunk_ev[i]);
        }
    }
    if (sink)
        if (int rc = sink->finish()) return rc;
    if (q.tot_host) {
        std::vector<uint64_t> t(nc * pcols);
        HIPCHK(hipMemcpyAsync(t.data(), b->totals.p, t.size() * 8, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        for (uint64_t col = 0; col < pcols; ++col) {
            uint64_t v = 0;
            for (size_t i = 0; i < nc; ++i) v += t[i * pcols + col];
            q.tot_host[col] = v;
        }
    }
    if (!q.dev) HIPCHK(hipStreamSynchronize(b->copy_stream));  // offs_h is rewritten by the next call
    if (narrowing) {  // a count wider than the wire (device reads: the caller's max_len understated)
        uint32_t over = 0;
        HIPCHK(hipMemcpyAsync(&over, b->ovf.p, sizeof(over), hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        if (over) return fail(XS_ERR_ARG, "a hit count does not fit %d byte(s): max_len is below the longest read",
                              wire);
    }
    return XS_OK;
}

}  // namespace

int xs::query_host(xs_bank* b, const HostQuery& q) {
    int wire = q.wire_bytes ? std::min(q.wire_bytes, q.hit_bytes) : q.hit_bytes;
    // a pinned destination takes the rows by DMA as they are
    if (q.hits_host && wire != q.hit_bytes && is_pinned_host(q.hits_host)) wire = q.hit_bytes;
    Chunks c;
    if (int rc = q.dev ? cut_dev_chunks(b, q, &c) : cut_host_chunks(b, q, &c)) return rc;
    if (int rc = reserve_host_query(b, q, c, wire)) return rc;
    return run_chunks(b, q, c, wire);
}

namespace {

// ---- small host calls ------------------------------------------------------------
// A request of a few reads (a serving loop's request, the per-read drop-in
// `search` of INTEGRATION.md §2) costs its launches, copies and syncs, not its
// probe: query_host's unit pipeline (units, scan, scatter), staging ring and
// three streams take 150-200 us for one read.  Here the host builds the unit
// map and packs the whole request into one pinned buffer: one H2D copy, the
// same direct probe kernel as query_host's gather path, one D2H copy of the
// per-block partials and the hit rows, one sync.  k-mer counts are the host's
// own (the formula of units_kernel), totals the sum of the partials.
constexpr uint64_t kSmallReads = 4096;
constexpr uint64_t kSmallBytes = 1u << 20;  // sequence bytes of the request
constexpr uint64_t kSmallUnits = 8192;
constexpr uint64_t kSmallUnitsPerBlock = 4;  // 4 waves taking 1 unit per grab (ReadView::grab)

size_t align16(size_t x) { return (x + 15) & ~size_t(15); }

// *done = false: the call does not qualify (nothing was enqueued).  Hit rows
// go to hits_host as hit_bytes-wide counts (the caller checked the width).
int query_small(xs_bank* b, const char* seqs, const uint64_t* offsets, uint64_t n, uint32_t step,
                void* hits_host, int hit_bytes, uint64_t* nk_host, uint64_t* tot_host, bool* done) {
    *done = false;
    if (b->profiling || n == 0 || n > kSmallReads || !b->opt.small_calls) return XS_OK;
    std::vector<uint64_t> ofs(n + 1);  // rebased to 0
    if (!rebase_offsets(offsets, n, ofs.data())) return bad_offsets();
    const uint64_t bytes = ofs[n];
    if (bytes > kSmallBytes) return XS_OK;
    const bool bloom = b->kind == XS_BANK_RBLOOM;
    const uint64_t cols = b->cols(), pcols = cols + 1;
    std::vector<uint64_t> nk(n), uofs(n + 1);
    uint64_t U = 0;
    bool zero_rows = false;  // rows the probe does not store whole (no k-mers, or several units)
    for (uint64_t r = 0; r < n; ++r) {
        const uint64_t len = ofs[r + 1] - ofs[r];
        nk[r] = sampled_kmers(len, b->k, step);
        const uint64_t s = (nk[r] + kSegKmers - 1) / kSegKmers;
        zero_rows |= s != 1;
        uofs[r] = U;
        U += s;
    }
    uofs[n] = U;
    if (U > kSmallUnits) return XS_OK;
    // only where query_host would take the direct / gather probe as well (a forced
    // or member-rich partitioned path keeps its own pipeline)
    if (bloom) poll_member_frac(b);
    if (bloom ? bloom_part_plan(b->bloom_view(), n, bytes, step, b->member_frac, b->opt)
              : cobs_part_plan(b->cobs_view(), b->k, n, bytes, step, b->opt))
        return XS_OK;
    const int blocks = (int)std::min<uint64_t>((uint64_t)probe_grid(b), std::max<uint64_t>(1, (U + kSmallUnitsPerBlock - 1) / kSmallUnitsPerBlock));
    // device / pinned layout: [queue | offsets | unit_ofs | unit_read | seqs] [partials | hits]
    const size_t o_off = 16, o_uofs = o_off + align16((n + 1) * 8), o_uread = o_uofs + align16((n + 1) * 8);
    const size_t o_seq = o_uread + align16(U * 4 + 4);
    const size_t in_bytes = o_seq + align16(bytes + kPad);
    const size_t o_part = in_bytes, part_bytes = align16((size_t)blocks * pcols * 8);
    const size_t o_hits = o_part + part_bytes;
    const size_t out_bytes = part_bytes + (hits_host ? n * cols * 4 : 0);
    if (int rc = b->small_h.ensure(in_bytes + out_bytes)) return rc;
    if (int rc = b->small_d.ensure(in_bytes + out_bytes)) return rc;
    char* h = static_cast<char*>(b->small_h.p);
    char* d = static_cast<char*>(b->small_d.p);
    auto* q = reinterpret_cast<uint64_t*>(h);
    q[0] = U;
    q[1] = 0;
    memcpy(h + o_off, ofs.data(), (n + 1) * 8);
    memcpy(h + o_uofs, uofs.data(), (n + 1) * 8);
    auto* ur = reinterpret_cast<uint32_t*>(h + o_uread);
    for (uint64_t r = 0; r < n; ++r)
        for (uint64_t u = uofs[r]; u < uofs[r + 1]; ++u) ur[u] = (uint32_t)r;
    if (bytes) memcpy(h + o_seq, seqs + offsets[0], bytes);
    memset(h + o_seq + bytes, 0, kPad);
    const hipStream_t s = b->stream;
    HIPCHK(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    uint32_t* d_hits = hits_host ? reinterpret_cast<uint32_t*>(d + o_hits) : nullptr;
    if (d_hits && zero_rows) HIPCHK(hipMemsetAsync(d_hits, 0, n * cols * 4, s));
    const ReadView rv{reinterpret_cast<const uint8_t*>(d + o_seq), bytes, reinterpret_cast<const uint64_t*>(d + o_off),
                      reinterpret_cast<const uint32_t*>(d + o_uread), reinterpret_cast<const uint64_t*>(d + o_uofs),
                      reinterpret_cast<uint64_t*>(d), n, b->k, step, /*grab=*/1};
    auto* d_part = reinterpret_cast<uint64_t*>(d + o_part);
    const char* kernel = "";
    if (bloom) HIPCHK(launch_probe_bloom(rv, b->bloom_view(), d_hits, d_part, blocks, s, &kernel));
    else HIPCHK(launch_probe_cobs(rv, b->cobs_view(), d_hits, d_part, blocks, s, &kernel));
    HIPCHK(hipMemcpyAsync(h + o_part, d + o_part, out_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    b->last_path = XS_PATH_GATHER;
    b->last_kernel = kernel;
    const auto* part = reinterpret_cast<const uint64_t*>(h + o_part);
    std::vector<uint64_t> tot(pcols, 0);
    for (int i = 0; i < blocks; ++i)
        for (uint64_t c = 0; c < pcols; ++c) tot[c] += part[(uint64_t)i * pcols + c];
    if (bloom) {  // the next query's path choice follows this one's member fraction
        if (tot[1]) b->member_frac = (double)tot[0] / (double)tot[1];
        b->bloom_pending = false;
    }
    if (tot_host) memcpy(tot_host, tot.data(), pcols * 8);
    if (nk_host) memcpy(nk_host, nk.data(), n * 8);
    if (hits_host) narrow_rows(hits_host, hit_bytes, reinterpret_cast<const uint32_t*>(h + o_hits), n * cols);
    *done = true;
    return XS_OK;
}

int build_impl(xs_bank* b, const Inputs& in, const uint32_t* d_doc, hipStream_t s) {
    if (int rc = ws_enter(b, s)) return rc;
    ReadView rv;
    if (int rc = prepare_units(b, in, 1, nullptr, nullptr, 0, s, &rv)) return rc;
    const int blocks = probe_grid(b);
    if (b->kind == XS_BANK_RBLOOM)
        HIPCHK(launch_build_bloom(rv, b->bloom_view(), b->image.as<uint32_t>(), blocks, s));
    else
        HIPCHK(launch_build_cobs(rv, d_doc, b->cobs_view(), b->image.as<uint32_t>(), blocks, s));
    return ws_leave(b, s);
}

// Hit rows for the host (hits_out, hit_bytes wide) and per-read k-mer counts: their device buffers.
int want_rows(xs_bank* b, HostQuery* q, void* hits_out, int hit_bytes, bool nk) {
    if (hits_out) {
        if (int rc = b->hits.ensure(q->n * b->cols() * 4)) return rc;
        q->d_hits = b->hits.as<uint32_t>();
        q->hits_host = hits_out;
        q->hit_bytes = hit_bytes;
    }
    if (int rc = nk ? b->nk.ensure(q->n * 8) : XS_OK) return rc;
    q->d_nk = nk ? b->nk.as<uint64_t>() : nullptr;
    return XS_OK;
}

int check_hit_bytes_step(int hit_bytes, uint32_t step) {
    if (hit_bytes != 1 && hit_bytes != 2 && hit_bytes != 4) return fail(XS_ERR_ARG, "hit_bytes must be 1, 2 or 4");
    if (step == 0) return fail(XS_ERR_ARG, "step must be >= 1");
    return XS_OK;
}

int query_impl(xs_bank* b, const char* seqs, const uint64_t* offsets, uint64_t n, uint32_t step,
               void* hits_out, int hit_bytes, uint64_t* num_kmers_out) {
    if (!b || !offsets || (!seqs && n)) return fail(XS_ERR_ARG, "null argument");
    if (int rc = check_hit_bytes_step(hit_bytes, step)) return rc;
    // a count never exceeds its read's sampled k-mers: they must fit the width, and
    // the rows cross PCIe in the narrowest width that holds the largest (wire_width)
    uint64_t max_nk = 0;
    if (hits_out) {
        const uint64_t cap = hit_bytes == 1 ? 0xFFu : hit_bytes == 2 ? 0xFFFFu : 0xFFFFFFFFu;
        uint64_t mx[8] = {}, over[8];
        for (auto& o : over) o = ~0ull;
        const uint32_t k = b->k;
        par_ranges(n, kSerialReads, host_threads(), [&](int t, uint64_t a, uint64_t e) {
            uint64_t m = 0;
            for (uint64_t r = a; r < e; ++r) {
                const uint64_t len = offsets[r + 1] >= offsets[r] ? offsets[r + 1] - offsets[r] : 0;
                const uint64_t nk = sampled_kmers(len, k, step);
                if (nk > cap && over[t] == ~0ull) over[t] = r;
                m = std::max(m, nk);
            }
            mx[t] = m;
        });
        for (int t = 0; t < 8; ++t) {
            if (over[t] != ~0ull) {
                const uint64_t r = over[t], len = offsets[r + 1] - offsets[r];
                return fail(XS_ERR_ARG, "read %llu has %llu sampled k-mers: counts may not fit %d byte(s)",
                            (unsigned long long)r, (unsigned long long)sampled_kmers(len, k, step), hit_bytes);
            }
            max_nk = std::max(max_nk, mx[t]);
        }
    }
    std::lock_guard<std::mutex> lk(b->mu);
    HIPCHK(hipSetDevice(b->device));
    if (n == 0) return XS_OK;
    bool done = false;
    if (int rc = query_small(b, seqs, offsets, n, step, hits_out, hit_bytes, num_kmers_out, nullptr, &done)) return rc;
    if (done) return XS_OK;
    HostQuery q{seqs, offsets, nullptr, n, step};
    if (int rc = want_rows(b, &q, hits_out, hit_bytes, num_kmers_out != nullptr)) return rc;
    q.wire_bytes = wire_width(max_nk, hit_bytes);
    if (int rc = query_host(b, q)) return rc;
    if (num_kmers_out) HIPCHK(hipMemcpyAsync(num_kmers_out, q.d_nk, n * 8, hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return XS_OK;
}

}  // namespace

extern "C" {

int xs_bank_build(xs_bank* b, const char* seqs, const uint64_t* offsets, const uint32_t* rec_doc,
                  uint64_t n_rec) {
    return xs::guard([&]() -> int {
        if (!b || (!seqs && n_rec) || !offsets) return fail(XS_ERR_ARG, "null argument");
        if (b->kind != XS_BANK_RBLOOM && n_rec && !rec_doc) return fail(XS_ERR_ARG, "rec_doc required");
        std::lock_guard<std::mutex> lk(b->mu);
        HIPCHK(hipSetDevice(b->device));
        if (n_rec == 0) return XS_OK;
        if (b->kind != XS_BANK_RBLOOM)
            for (uint64_t r = 0; r < n_rec; ++r)
                if (rec_doc[r] >= b->D) return fail(XS_ERR_ARG, "rec_doc[%llu] out of range", (unsigned long long)r);
        Inputs in;
        if (int rc = upload_reads(b, seqs, offsets, n_rec, b->stream, &in)) return rc;
        HIPCHK(hipStreamSynchronize(b->stream));  // the caller's reads are on the device (or in the ring) from here
        uint32_t* d_doc = nullptr;
        if (b->kind != XS_BANK_RBLOOM) {
            if (int rc = b->tmp.ensure(n_rec * 4)) return rc;
            d_doc = b->tmp.as<uint32_t>();
            HIPCHK(hipMemcpyAsync(d_doc, rec_doc, n_rec * 4, hipMemcpyHostToDevice, b->stream));
        }
        if (int rc = build_impl(b, in, d_doc, b->stream)) return rc;
        HIPCHK(hipStreamSynchronize(b->stream));
        return XS_OK;
    });
}

int xs_bank_build_device(xs_bank* b, const void* d_seqs, uint64_t seq_bytes,
                         const uint64_t* d_offsets, const uint32_t* d_rec_doc, uint64_t n_rec,
                         void* stream) {
    return xs::guard([&]() -> int {
        if (!b || !d_offsets) return fail(XS_ERR_ARG, "null argument");
        if (b->kind != XS_BANK_RBLOOM && n_rec && !d_rec_doc) return fail(XS_ERR_ARG, "rec_doc required");
        std::lock_guard<std::mutex> lk(b->mu);
        HIPCHK(hipSetDevice(b->device));
        if (n_rec == 0) return XS_OK;
        Inputs in{static_cast<const uint8_t*>(d_seqs), seq_bytes, d_offsets, n_rec};
        hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null (legacy default) stream
        return build_impl(b, in, d_rec_doc, s);
    });
}

int xs_query(xs_bank* b, const char* seqs, const uint64_t* offsets, uint64_t n, uint32_t step,
             uint32_t* hits_out, uint64_t* num_kmers_out) {
    return xs::guard([&]() -> int {
        return query_impl(b, seqs, offsets, n, step, hits_out, 4, num_kmers_out);
    });
}

int xs_query_hits(xs_bank* b, const char* seqs, const uint64_t* offsets, uint64_t n, uint32_t step,
                  void* hits_out, int hit_bytes, uint64_t* num_kmers_out) {
    return xs::guard([&]() -> int {
        return query_impl(b, seqs, offsets, n, step, hits_out, hit_bytes, num_kmers_out);
    });
}

int xs_query_hits_device(xs_bank* b, const void* d_seqs, uint64_t seq_bytes, const uint64_t* d_offsets, uint64_t n,
                         uint64_t max_len, uint32_t step, void* hits_out, int hit_bytes, uint64_t* num_kmers_out,
                         uint64_t* totals_out) {
    return xs::guard([&]() -> int {
        if (!b || (n && (!d_seqs || !d_offsets))) return fail(XS_ERR_ARG, "null argument");
        if (int rc = check_hit_bytes_step(hit_bytes, step)) return rc;
        const uint64_t max_nk = sampled_kmers(max_len, b->k, step);
        if (hits_out && hit_bytes != 4) {
            const uint64_t cap = hit_bytes == 1 ? 0xFFu : 0xFFFFu;
            if (max_nk > cap)
                return fail(XS_ERR_ARG, "a read has %llu sampled k-mers: counts may not fit %d byte(s)",
                            (unsigned long long)max_nk, hit_bytes);
        }
        std::lock_guard<std::mutex> lk(b->mu);
        HIPCHK(hipSetDevice(b->device));
        const uint64_t cols = b->cols();
        if (n == 0) {
            if (totals_out) memset(totals_out, 0, (cols + 1) * 8);
            return XS_OK;
        }
        const DevReads dev{static_cast<const uint8_t*>(d_seqs), seq_bytes, d_offsets};
        HostQuery q{nullptr, nullptr, &dev, n, step};
        if (int rc = want_rows(b, &q, hits_out, hit_bytes, num_kmers_out != nullptr)) return rc;
        std::vector<uint64_t> tot(totals_out ? cols + 1 : 0);
        if (totals_out) q.tot_host = tot.data();
        if (int rc = query_host(b, q)) return rc;
        if (num_kmers_out) HIPCHK(hipMemcpyAsync(num_kmers_out, b->nk.p, n * 8, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        if (totals_out) memcpy(totals_out, tot.data(), (cols + 1) * 8);
        return XS_OK;
    });
}

int xs_query_best(xs_bank* b, const char* seqs, const uint64_t* offsets, uint64_t n, uint32_t step,
                  uint32_t* best_doc, uint32_t* best_hits, uint64_t* num_kmers_out, uint64_t* totals_out) {
    return xs::guard([&]() -> int {
        if (!b || !offsets || ((!seqs || !best_doc) && n)) return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(b->mu);
        HIPCHK(hipSetDevice(b->device));
        const uint64_t cols = b->cols();
        if (n == 0) {
            if (totals_out) memset(totals_out, 0, (cols + 1) * 8);
            return XS_OK;
        }
        if (n <= kSmallReads && n * cols <= (1u << 16)) {  // a small request: the per-read call made on the host
            std::vector<uint32_t> rows(n * cols);
            std::vector<uint64_t> tot(cols + 1);
            bool done = false;
            if (int rc = query_small(b, seqs, offsets, n, step, rows.data(), 4, num_kmers_out, tot.data(), &done)) return rc;
            if (done) {
                best_rows(rows.data(), n, cols, best_doc, best_hits);
                if (totals_out) memcpy(totals_out, tot.data(), (cols + 1) * 8);
                return XS_OK;
            }
        }
        if (int rc = b->hits.ensure(n * cols * 4)) return rc;
        if (int rc = b->nk.ensure(n * 8)) return rc;
        if (int rc = b->best.ensure(n * 8)) return rc;
        uint32_t* d_hits = b->hits.as<uint32_t>();
        uint32_t* d_best = b->best.as<uint32_t>();
        uint32_t* d_bhits = d_best + n;
        std::vector<uint64_t> tot(totals_out ? cols + 1 : 0);
        HostQuery q{seqs, offsets, nullptr, n, step};
        q.d_hits = d_hits;
        q.d_nk = b->nk.as<uint64_t>();
        if (totals_out) q.tot_host = tot.data();
        if (int rc = query_host(b, q)) return rc;
        HIPCHK(launch_best_doc(d_hits, n, cols, d_best, d_bhits, b->stream));
        HIPCHK(hipMemcpyAsync(best_doc, d_best, n * 4, hipMemcpyDeviceToHost, b->stream));
        if (best_hits) HIPCHK(hipMemcpyAsync(best_hits, d_bhits, n * 4, hipMemcpyDeviceToHost, b->stream));
        if (num_kmers_out)
            HIPCHK(hipMemcpyAsync(num_kmers_out, b->nk.p, n * 8, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        if (totals_out) memcpy(totals_out, tot.data(), (cols + 1) * 8);
        return XS_OK;
    });
}

int xs_query_keep(xs_bank* b, const char* seqs, const uint64_t* offsets, uint64_t n, uint32_t step, uint64_t label_doc,
                  const uint8_t* doc_mask, double threshold, uint8_t* keep_out, uint32_t* label_hits_out,
                  uint64_t* num_kmers_out, uint64_t* totals_out) {
    return xs::guard([&]() -> int {
        if (!b || !offsets || ((!seqs || !keep_out) && n)) return fail(XS_ERR_ARG, "null argument");
        int c_min = 0;
        if (!filter_mode(threshold, &c_min)) return fail(XS_ERR_ARG, "threshold must be in [0, 1] or -1");
        const uint64_t cols = b->cols();
        if (label_doc >= cols) return fail(XS_ERR_ARG, "label_doc out of range");
        if (doc_mask && !doc_mask[label_doc]) return fail(XS_ERR_ARG, "label_doc is masked out");
        std::lock_guard<std::mutex> lk(b->mu);
        HIPCHK(hipSetDevice(b->device));
        if (n == 0) {
            if (totals_out) memset(totals_out, 0, (cols + 1) * 8);
            return XS_OK;
        }
        if (n <= kSmallReads && n * cols <= (1u << 16)) {  // a small request: the decision made on the host
            std::vector<uint32_t> rows(n * cols);
            std::vector<uint64_t> nk(n), tot(cols + 1);
            bool done = false;
            if (int rc = query_small(b, seqs, offsets, n, step, rows.data(), 4, nk.data(), tot.data(), &done)) return rc;
            if (done) {
                filter_keep_rows(rows.data(), nk.data(), n, cols, label_doc, doc_mask, c_min, keep_out, label_hits_out);
                if (num_kmers_out) memcpy(num_kmers_out, nk.data(), n * 8);
                if (totals_out) memcpy(totals_out, tot.data(), (cols + 1) * 8);
                return XS_OK;
            }
        }
        if (int rc = b->hits.ensure(n * cols * 4)) return rc;
        if (int rc = b->nk.ensure(n * 8)) return rc;
        if (int rc = b->best.ensure(n * 5)) return rc;  // the label's hits, then the keep bytes
        uint32_t* d_hits = b->hits.as<uint32_t>();
        uint32_t* d_lh = b->best.as<uint32_t>();
        uint8_t* d_keep = reinterpret_cast<uint8_t*>(d_lh + n);
        uint8_t* d_mask = nullptr;
        if (doc_mask && c_min < 0) {  // only the row maximum of max mode reads it
            if (int rc = b->tmp.ensure(cols)) return rc;
            d_mask = b->tmp.as<uint8_t>();
        }
        std::vector<uint64_t> tot(totals_out ? cols + 1 : 0);
        HostQuery q{seqs, offsets, nullptr, n, step};
        q.d_hits = d_hits;
        q.d_nk = b->nk.as<uint64_t>();
        if (totals_out) q.tot_host = tot.data();
        if (int rc = query_host(b, q)) return rc;
        if (d_mask) HIPCHK(hipMemcpyAsync(d_mask, doc_mask, cols, hipMemcpyHostToDevice, b->stream));
        HIPCHK(launch_filter_keep(d_hits, q.d_nk, n, cols, label_doc, d_mask, c_min, d_keep, d_lh, b->stream));
        HIPCHK(hipMemcpyAsync(keep_out, d_keep, n, hipMemcpyDeviceToHost, b->stream));
        if (label_hits_out) HIPCHK(hipMemcpyAsync(label_hits_out, d_lh, n * 4, hipMemcpyDeviceToHost, b->stream));
        if (num_kmers_out)
            HIPCHK(hipMemcpyAsync(num_kmers_out, b->nk.p, n * 8, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipStreamSynchronize(b->stream));
        if (totals_out) memcpy(totals_out, tot.data(), (cols + 1) * 8);
        return XS_OK;
    });
}

int xs_query_totals(xs_bank* b, const char* seqs, const uint64_t* offsets, uint64_t n,
                    uint32_t step, uint64_t* totals_out, uint64_t* total_kmers_out) {
    return xs::guard([&]() -> int {
        if (!b || !offsets || (!seqs && n) || !totals_out) return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(b->mu);
        HIPCHK(hipSetDevice(b->device));
        const uint64_t cols = b->cols();
        if (n == 0) {
            memset(totals_out, 0, cols * 8);
            if (total_kmers_out) *total_kmers_out = 0;
            return XS_OK;
        }
        std::vector<uint64_t> t(cols + 1);
        bool done = false;
        if (int rc = query_small(b, seqs, offsets, n, step, nullptr, 4, nullptr, t.data(), &done)) return rc;
        if (!done) {
            HostQuery q{seqs, offsets, nullptr, n, step};
            q.tot_host = t.data();
            if (int rc = query_host(b, q)) return rc;
        }
        memcpy(totals_out, t.data(), cols * 8);
        if (total_kmers_out) *total_kmers_out = t[cols];
        return XS_OK;
    });
}

int xs_query_device(xs_bank* b, const void* d_seqs, uint64_t seq_bytes, const uint64_t* d_offsets,
                    uint64_t n, uint32_t step, uint32_t* d_hits, uint64_t* d_num_kmers,
                    uint64_t* d_totals, void* stream) {
    return xs::guard([&]() -> int {
        if (!b || !d_offsets || (!d_seqs && n)) return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(b->mu);
        HIPCHK(hipSetDevice(b->device));
        hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = the null (legacy default) stream
        if (n == 0) {
            if (d_totals) HIPCHK(hipMemsetAsync(d_totals, 0, (b->cols() + 1) * 8, s));
            return XS_OK;
        }
        Inputs in{static_cast<const uint8_t*>(d_seqs), seq_bytes, d_offsets, n};
        return run_query(b, in, step, d_hits, d_num_kmers, d_totals, s);
    });
}

}  // extern "C"
