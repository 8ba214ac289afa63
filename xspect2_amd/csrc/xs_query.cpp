// xs_query.cpp — queries and builds on a bank handle: the probe dispatcher (run_query), the chunked
// host pipeline (query_host), the small-call path (query_small) and their C ABI entry points.
#include <memory>

#include "xs_hitsink.h"
#include "xs_host.h"

using namespace xs;

namespace {

// ---- query / build pipeline --------------------------------------------------
struct Inputs {
    const uint8_t* seqs;
    uint64_t seq_bytes;      // readable bytes from seqs (window loads stop there)
    const uint64_t* offs;
    uint64_t n;
    uint64_t read_bytes = 0;  // bytes of these n reads (plans and bounds); 0: seq_bytes
    uint64_t plan_bytes() const { return read_bytes ? read_bytes : seq_bytes; }
};

// Unit decomposition (k-mer counts, units, unit -> read map) for n device-resident reads.
// units = false (the partitioned COBS probe, which maps k-mers to reads itself and
// zeroes the hit matrix): only the per-read k-mer counts, when the caller wants them.
int prepare_units(xs_bank* b, const Inputs& in, uint32_t step, uint64_t* d_nk, uint32_t* hits_zero,
                  uint64_t zero_cols, hipStream_t s, ReadView* rv, bool units = true) {
    if (int rc = b->nseg.ensure((in.n + 1) * 8)) return rc;
    if (int rc = b->unit_ofs.ensure((in.n + 1) * 8)) return rc;
    if (int rc = b->n_units.ensure(2 * sizeof(uint64_t))) return rc;
    const uint64_t unit_bound = in.n + in.plan_bytes() / kSegKmers + 1;
    if (int rc = b->unit_read.ensure(unit_bound * 4)) return rc;
    const size_t tb = scan_temp_bytes(in.n ? in.n : 1);
    if (int rc = b->scan_tmp.ensure(tb)) return rc;
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
// the direct / gather probe instead of failing (false).  miss = 0 (COBS): no miss bitmap.
bool reserve_part_ws(xs_bank* b, size_t nkc, size_t scan, size_t entry, size_t tbl, size_t miss, size_t aux) {
    if (b->pk_nkc.ensure(nkc) || b->pk_kofs.ensure(nkc) || b->pk_scan.ensure(scan) || b->pk_entries.ensure(entry) ||
        b->pk_tbl.ensure(tbl) || (miss && b->pk_miss.ensure(miss)) || b->pk_aux.ensure(aux)) {
        (void)hipGetLastError();
        return false;
    }
    return true;
}

// Enqueue one query on device buffers.  d_totals: cols() + 1 entries.
int run_query(xs_bank* b, const Inputs& in, uint32_t step, uint32_t* d_hits, uint64_t* d_nk,
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
                    reserve_part_ws(b, cplan.nkc_bytes, cplan.scan_bytes, cplan.entry_bytes, cplan.tbl_bytes, 0,
                                    cplan.aux_bytes);
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
    if (bloom && bloom_part_plan(b->bloom_view(), in.n, in.plan_bytes(), step, b->member_frac, b->opt, &plan) &&
        reserve_part_ws(b, plan.nkc_bytes, plan.scan_bytes, plan.entry_bytes, plan.tbl_bytes, plan.miss_bytes,
                        plan.aux_bytes)) {
        path = XS_PATH_PARTITIONED;
        kernel = "bloompart";
        const BloomPartWs ws{b->pk_nkc.as<uint64_t>(), b->pk_kofs.as<uint64_t>(), b->pk_scan.p, b->pk_scan.cap,
                             b->pk_entries.as<uint64_t>(), b->pk_tbl.as<uint16_t>(), b->pk_miss.as<uint32_t>(),
                             b->pk_aux.as<uint32_t>()};
        PassRecorder rec{&b->pass_ev, &b->pass_tag, &b->pass_used};
        HIPCHK(launch_probe_bloom_part(rv, b->bloom_view(), plan, ws, d_hits, partials, blocks, s,
                                       b->profiling ? &rec : nullptr));
    } else if (bloom) {
        HIPCHK(launch_probe_bloom(rv, b->bloom_view(), d_hits, partials, blocks, s, &kernel));
    } else {
        const CobsView cv = b->cobs_view();
        if (cobs_part) {
            path = XS_PATH_PARTITIONED;
            kernel = "cobspart";
            const PartWs ws{b->pk_nkc.as<uint64_t>(), b->pk_kofs.as<uint64_t>(), b->pk_scan.p, b->pk_scan.cap,
                            b->pk_entries.p, b->pk_tbl.as<uint16_t>(), b->pk_aux.as<uint32_t>()};
            PassRecorder rec{&b->pass_ev, &b->pass_tag, &b->pass_used};
            HIPCHK(launch_probe_cobs_part(rv, cv, cplan, ws, d_hits, partials, blocks, s, b->profiling ? &rec : nullptr));
        } else {
            HIPCHK(launch_probe_cobs(rv, cv, d_hits, partials, blocks, s, &kernel));
        }
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

// A host batch's per-read passes run before its first copy, in the call's critical path: on
// one thread below kSerialReads reads.  dst[r] = offsets[r] - offsets[0] for the n + 1 offsets of n reads, in one pass on several
// threads; false when a pair of offsets decreases
constexpr uint64_t kSerialReads = 1u << 18;
bool rebase_offsets(const uint64_t* offsets, uint64_t n, uint64_t* dst) {
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
int bad_offsets() { return fail(XS_ERR_ARG, "offsets must be non-decreasing"); }

// Copy host reads to the handle's device buffers (offsets rebased to 0).
int stage_host_reads(xs_bank* b, const char* seqs, const uint64_t* offsets, uint64_t n, Inputs* in) {
    const uint64_t bytes = offsets[n] - offsets[0];
    std::vector<uint64_t> rebased(n + 1);
    if (!rebase_offsets(offsets, n, rebased.data())) return bad_offsets();
    if (int rc = b->seqs.ensure(bytes + kPad)) return rc;
    if (int rc = b->offs.ensure((n + 1) * 8)) return rc;
    if (bytes) HIPCHK(hipMemcpyAsync(b->seqs.p, seqs + offsets[0], bytes, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->offs.p, rebased.data(), (n + 1) * 8, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));  // `rebased` leaves scope
    *in = Inputs{b->seqs.as<uint8_t>(), bytes, b->offs.as<uint64_t>(), n};
    return XS_OK;
}

// Device -> pageable host copy of `bytes`, ordered after the work already on
// stream `st`.  Large copies go through a pinned two-slot ring: the DMA of
// chunk i overlaps the host copy of chunk i-1 (a plain pageable D2H runs at
// about 9 GB/s on the box, a pinned one at PCIe rate).  Returns once the data
// is in `host`.
int d2h_pageable(xs_bank* b, void* host, const void* dev, size_t bytes, hipStream_t st) {
    constexpr size_t kChunk = 32u << 20;
    if (bytes < 2 * kChunk || is_pinned_host(host)) {
        HIPCHK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return XS_OK;
    }
    for (int s = 0; s < 2; ++s) {
        if (int rc = b->stage[s].ensure(kChunk)) return rc;
        if (!b->stage_ev[s]) HIPCHK(hipEventCreateWithFlags(&b->stage_ev[s], hipEventDisableTiming));
    }
    const int threads = host_threads();
    size_t prev_off = 0, prev_n = 0;
    int prev_slot = -1;
    for (size_t off = 0, i = 0; off < bytes; off += kChunk, ++i) {
        const int slot = (int)(i & 1);
        const size_t n = std::min(kChunk, bytes - off);
        HIPCHK(hipMemcpyAsync(b->stage[slot].p, static_cast<const char*>(dev) + off, n, hipMemcpyDeviceToHost,
                              st));
        HIPCHK(hipEventRecord(b->stage_ev[slot], st));
        if (prev_slot >= 0) {
            HIPCHK(hipEventSynchronize(b->stage_ev[prev_slot]));
            par_memcpy(static_cast<char*>(host) + prev_off, b->stage[prev_slot].p, prev_n, threads);
        }
        prev_off = off;
        prev_n = n;
        prev_slot = slot;
    }
    HIPCHK(hipEventSynchronize(b->stage_ev[prev_slot]));
    par_memcpy(static_cast<char*>(host) + prev_off, b->stage[prev_slot].p, prev_n, threads);
    return XS_OK;
}

// ---- host batches: staging overlapped with the probe --------------------------
// A host batch is cut at read boundaries into chunks of about kHostChunk
// sequence bytes (the first smaller, so the probe starts early).  Chunk i is
// copied into a pinned slot by host threads and sent on the copy stream while
// the bank stream probes chunk i-1.  With host hits wanted, chunk i-1's hit
// rows go back through the D2H ring on a third stream while chunk i is probed
// (HitSink).  Device buffers span the whole batch, so chunks never overwrite
// each other's reads or hits, and the workspace is sized for the whole batch up
// front (no reallocation, hence no implicit device sync, between chunks).
constexpr size_t kHostChunk = 32u << 20;
constexpr size_t kHostFirst = 8u << 20;

// Reads already in HBM (a device-mode reader's batch): query_host then only
// chunks the probe and the hit-row D2H.
struct DevReads {
    const uint8_t* seqs;
    uint64_t seq_bytes;
    const uint64_t* offs;  // n+1, offs[0] = 0
};
constexpr uint64_t kDevChunkReads = 1u << 18;

// One call of query_host: where the n reads are, and what the caller wants back.
struct HostQuery {
    const char* seqs;         // reads on the host: their bytes and n + 1 offsets as the caller gave them ...
    const uint64_t* offsets;
    const DevReads* dev;      // ... or reads on the device (seqs and offsets null); chunks are then cut by read count
    uint64_t n;
    uint32_t step;
    uint32_t* d_hits = nullptr;    // n x cols uint32 rows on the device
    // the rows back on the host (needs d_hits) as hit_bytes-wide counts, crossing PCIe wire_bytes wide (0: hit_bytes;
    // narrower: narrowed on the device into b->narrow, widened on the host; the caller checked that they fit)
    void* hits_host = nullptr;
    int hit_bytes = 4, wire_bytes = 0;
    uint64_t* d_nk = nullptr;      // per-read k-mer counts on the device
    uint64_t* tot_host = nullptr;  // cols + 1 entries on the host: per-doc sums, then the k-mer total
};

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
    if (int rc = b->nseg.ensure((n + 1) * 8)) return rc;
    if (int rc = b->unit_ofs.ensure((n + 1) * 8)) return rc;
    if (int rc = b->n_units.ensure(2 * sizeof(uint64_t))) return rc;
    if (int rc = b->unit_read.ensure((n + c.bytes / kSegKmers + 1) * 4)) return rc;
    if (int rc = b->scan_tmp.ensure(scan_temp_bytes(n))) return rc;
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
    struct DrainOnExit {
        hipStream_t s = nullptr;
        ~DrainOnExit() {
            if (s) (void)hipStreamSynchronize(s);
        }
    } drain;
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

int query_host(xs_bank* b, const HostQuery& q) {
    int wire = q.wire_bytes ? std::min(q.wire_bytes, q.hit_bytes) : q.hit_bytes;
    // a pinned destination takes the rows by DMA as they are
    if (q.hits_host && wire != q.hit_bytes && is_pinned_host(q.hits_host)) wire = q.hit_bytes;
    Chunks c;
    if (int rc = q.dev ? cut_dev_chunks(b, q, &c) : cut_host_chunks(b, q, &c)) return rc;
    if (int rc = reserve_host_query(b, q, c, wire)) return rc;
    return run_chunks(b, q, c, wire);
}

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
        nk[r] = len >= b->k ? (len - b->k) / step + 1 : 0;
        const uint64_t s = (nk[r] + kSegKmers - 1) / kSegKmers;
        zero_rows |= s != 1;
        uofs[r] = U;
        U += s;
    }
    uofs[n] = U;
    if (U > kSmallUnits) return XS_OK;
    // only where query_host would take the direct / gather probe as well (a forced
    // or member-rich partitioned path keeps its own pipeline)
    if (bloom) {
        poll_member_frac(b);
        BloomPartPlan plan;
        if (bloom_part_plan(b->bloom_view(), n, bytes, step, b->member_frac, b->opt, &plan)) return XS_OK;
    } else {
        CobsPartPlan plan;
        if (cobs_part_plan(b->cobs_view(), b->k, n, bytes, step, b->opt, &plan)) return XS_OK;
    }
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

int query_impl(xs_bank* b, const char* seqs, const uint64_t* offsets, uint64_t n, uint32_t step,
               void* hits_out, int hit_bytes, uint64_t* num_kmers_out) {
    if (!b || !offsets || (!seqs && n)) return fail(XS_ERR_ARG, "null argument");
    if (hit_bytes != 1 && hit_bytes != 2 && hit_bytes != 4) return fail(XS_ERR_ARG, "hit_bytes must be 1, 2 or 4");
    if (step == 0) return fail(XS_ERR_ARG, "step must be >= 1");
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
                const uint64_t nk = len >= k ? (len - k) / step + 1 : 0;
                if (nk > cap && over[t] == ~0ull) over[t] = r;
                m = std::max(m, nk);
            }
            mx[t] = m;
        });
        for (int t = 0; t < 8; ++t) {
            if (over[t] != ~0ull) {
                const uint64_t r = over[t], len = offsets[r + 1] - offsets[r];
                return fail(XS_ERR_ARG, "read %llu has %llu sampled k-mers: counts may not fit %d byte(s)",
                            (unsigned long long)r, (unsigned long long)((len - k) / step + 1), hit_bytes);
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

// ---- MLST typing: every locus of a scheme, rows reduced on the device -----------
// The reads are in HBM once (uploaded into the first locus' buffers, or a device reader's batch).
// They are probed in chunks of R reads, R x Dmax x 4 <= the workspace: per chunk and locus the
// probe fills the rows buffer and mlst_top_kernel reduces it into column l of the n x loci device
// outputs, so the rows buffer does not grow with n and no hit matrix crosses PCIe.  Everything
// runs on the first locus' stream; its buffers hold the reads, the rows and the outputs.
constexpr uint64_t kMlstTypeWs = 4ull << 30;  // default cap of the rows buffer

struct MlstTypeOut {
    uint32_t *top, *top_score, *n_tied;  // n x loci each, host (n_tied may be null)
    uint64_t* num_kmers;                 // n, host (may be null)
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

// Every locus' mutex, taken in address order: two calls over the same handles in any order cannot deadlock.
struct LociLock {
    std::vector<std::unique_lock<std::mutex>> held;
    LociLock(xs_bank* const* loci, uint32_t n_loci) {
        std::vector<xs_bank*> order(loci, loci + n_loci);
        std::sort(order.begin(), order.end(), std::less<xs_bank*>());
        for (xs_bank* b : order) held.emplace_back(b->mu);
    }
};

// Host reads into b's device buffers on stream s (offsets rebased to 0, kept in b->offs_h for the
// call): pageable bytes go through the pinned H2D ring, the copy of slot i behind the host's fill of
// slot i+1.  The caller synchronises s before the source memory may change.
int upload_reads(xs_bank* b, const char* seqs, const uint64_t* offsets, uint64_t n, hipStream_t s, Inputs* in) {
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

// Several device regions -> host memory, ordered after the work already on `st`; returns once
// they are there.  d2h_pageable's ring over all the parts: a part of kD2hRingMin bytes or more
// bound for pageable memory crosses in 32 MiB pieces through the two pinned slots, the DMA of one
// piece behind the host threads' copy of the one before; the others are plain copies.
struct D2hPart {
    void* host;
    const void* dev;
    size_t bytes;
};
constexpr size_t kD2hRingMin = 1u << 20;
int d2h_parts(xs_bank* b, const D2hPart* parts, int n_parts, hipStream_t st) {
    constexpr size_t kChunk = 32u << 20;
    const int threads = host_threads();
    char* prev_host = nullptr;
    size_t prev_n = 0, i = 0;
    int prev_slot = -1;
    for (int p = 0; p < n_parts; ++p) {
        const D2hPart& part = parts[p];
        if (!part.bytes) continue;
        if (part.bytes < kD2hRingMin || is_pinned_host(part.host)) {
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

// The chunks, probes and reductions of one call, enqueued on the first locus' stream; then the
// outputs' copies to the host.  host_offs: the reads' offsets on the host (n + 1, [0] = 0) or null.
int mlst_type_run(xs_bank* const* loci, uint32_t n_loci, const Inputs& all, const uint64_t* host_offs, uint32_t step,
                  uint64_t workspace_bytes, const MlstTypeOut& out) {
    xs_bank* b0 = loci[0];
    const hipStream_t s = b0->stream;
    const uint64_t n = all.n, L = n_loci;
    uint64_t dmax = 1;
    for (uint32_t l = 0; l < n_loci; ++l) dmax = std::max(dmax, loci[l]->D);
    const uint64_t ws = workspace_bytes ? workspace_bytes : kMlstTypeWs;
    const uint64_t per = std::min<uint64_t>({std::max<uint64_t>(1, ws / (dmax * 4)), n, (1ull << 31) - 1});
    if (int rc = ws_enter(b0, s)) return rc;
    if (int rc = b0->hits.ensure(per * dmax * 4)) return rc;
    if (int rc = b0->best.ensure(n * L * 4 * 3)) return rc;
    if (out.num_kmers)
        if (int rc = b0->nk.ensure(n * 8)) return rc;
    uint32_t* d_rows = b0->hits.as<uint32_t>();
    uint32_t* d_top = b0->best.as<uint32_t>();
    uint32_t* d_score = d_top + n * L;
    uint32_t* d_tied = out.n_tied ? d_score + n * L : nullptr;
    uint64_t* d_nk = out.num_kmers ? b0->nk.as<uint64_t>() : nullptr;
    for (uint64_t r0 = 0; r0 < n; r0 += per) {
        const uint64_t cn = std::min(per, n - r0);
        // the chunk's own bytes where the host knows the offsets; else the batch's, an upper bound (plans only)
        const Inputs in{all.seqs, all.seq_bytes, all.offs + r0, cn, host_offs ? host_offs[r0 + cn] - host_offs[r0] : 0};
        for (uint32_t l = 0; l < n_loci; ++l) {
            if (int rc = run_query(loci[l], in, step, d_rows, l == 0 && d_nk ? d_nk + r0 : nullptr, nullptr, s)) return rc;
            const uint64_t o = r0 * L + l;
            HIPCHK(launch_mlst_top(d_rows, cn, loci[l]->D, d_top + o, d_score + o, d_tied ? d_tied + o : nullptr, L, s));
        }
    }
    if (int rc = ws_leave(b0, s)) return rc;
    const D2hPart parts[4] = {{out.top, d_top, n * L * 4},
                              {out.top_score, d_score, n * L * 4},
                              {out.n_tied, d_tied, d_tied ? n * L * 4 : 0},
                              {out.num_kmers, d_nk, d_nk ? n * 8 : 0}};
    return d2h_parts(b0, parts, 4, s);
}

// However a call ends, nothing enqueued for it may still read the caller's reads once it has returned.
struct DrainStream {
    hipStream_t s;
    ~DrainStream() { (void)hipStreamSynchronize(s); }
};

// ---- MLST typing of contigs: chunked, probed, summed and reduced on the device ----
// Records of long_len bytes and more follow the reference's chunk rule (xspect_hip.h), the others
// mlst_type_run's.  Short records are probed where they lie, run by run of consecutive records (or,
// when a batch interleaves so many runs that their launches would dominate, compacted once by
// gather_reads_kernel and their outputs scattered back).  Per locus the long records' chunks are
// numbered through and processed in ranges of at most R chunks (R rows of the widest locus within
// the workspace) and about as many text bytes: the splitter writes the range's chunk texts, the
// probe its rows, one pass adds them to the per-record accumulators and a wave per finished record
// writes its call.  A record cut by a range end keeps its accumulators in slot 0 of the next range.
// The host's part is the chunk runs, closed forms of the lengths: O(long records + ranges) per locus.
constexpr xs_mlst_chunk_rule_t kReferenceRule{10000, 1000000, 10000000, 50, 0};
constexpr size_t kMaxShortRuns = 64;  // more runs of short records than this: compact them first

int chunk_rule_check(const xs_mlst_chunk_rule_t* rule, xs_mlst_chunk_rule_t* out) {
    *out = rule ? *rule : kReferenceRule;
    if (out->scale10_len > out->scale100_len) return fail(XS_ERR_ARG, "scale10_len must be <= scale100_len");
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

// n reads [r0, r0 + n) probed against every locus in pieces of `per` reads, each piece's rows reduced into
// columns of the outputs whose row 0 is the first read's (top / score / tied point at it).
int mlst_type_span(xs_bank* const* loci, uint32_t n_loci, const Inputs& all, const uint64_t* ho, uint64_t r0, uint64_t n,
                   uint64_t per, uint32_t step, uint32_t* d_rows, uint32_t* top, uint32_t* score, uint32_t* tied,
                   hipStream_t s) {
    const uint64_t L = n_loci;
    for (uint64_t a = 0; a < n; a += per) {
        const uint64_t cn = std::min(per, n - a);
        const Inputs in{all.seqs, all.seq_bytes, all.offs + r0 + a, cn, ho[r0 + a + cn] - ho[r0 + a]};
        for (uint32_t l = 0; l < n_loci; ++l) {
            if (int rc = run_query(loci[l], in, step, d_rows, nullptr, nullptr, s)) return rc;
            const uint64_t o = a * L + l;
            HIPCHK(launch_mlst_top(d_rows, cn, loci[l]->D, top + o, score + o, tied ? tied + o : nullptr, L, s));
        }
    }
    return XS_OK;
}

// One range of one locus: runs [run0, run0 + n_runs) of the call's run array (a sentinel follows them).
struct ChunkRange {
    uint64_t run0, n_runs, nc, bytes, chunk_base;
    bool carry_in, carry_out;  // its first run continues a record / its last run's record goes on
};

// The ranges of one locus appended to `ranges`, their runs to `runs`.  ho: the reads' host offsets.
void cut_chunk_ranges(const std::vector<uint64_t>& longs, const uint64_t* ho, uint64_t w, uint32_t k,
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
            const uint64_t take = std::min({g.chunks - j, row_cap - cu, fit});
            if (take == 0) {
                close(j > 0);
                continue;
            }
            const bool to_end = j + take == g.chunks;
            const uint64_t nb = to_end ? (take - 1) * W + mlst_chunk_len(g, n, W, k, g.chunks - 1) : take * W;
            runs->push_back(MlstChunkRun{cu, ho[rec], n, W, j, bu, rec, 0});
            cu += take;
            bu += nb;
            j += take;
        }
    }
    if (cu) close(false);
}

int mlst_contigs_run(xs_bank* const* loci, uint32_t n_loci, const uint64_t* width, const xs_mlst_chunk_rule_t& rule,
                     const Inputs& all, const uint64_t* ho, uint32_t step, uint64_t workspace_bytes,
                     const MlstTypeOut& out) {
    xs_bank* b0 = loci[0];
    const hipStream_t s = b0->stream;
    const uint64_t n = all.n, L = n_loci;
    const uint32_t k = b0->k;
    uint64_t dmax = 1;
    for (uint32_t l = 0; l < n_loci; ++l) dmax = std::max(dmax, loci[l]->D);
    const uint64_t ws = workspace_bytes ? workspace_bytes : kMlstTypeWs;
    const uint64_t row_cap = std::min<uint64_t>(std::max<uint64_t>(1, ws / (dmax * 4)), (1ull << 31) - 1);

    // the records by kind: the long ones, and the runs of consecutive short ones
    std::vector<uint64_t> longs;
    std::vector<std::pair<uint64_t, uint64_t>> short_runs;
    uint64_t n_short = 0, short_bytes = 0;
    for (uint64_t r = 0, run = 0; r <= n; ++r) {
        const bool is_long = r < n && ho[r + 1] - ho[r] >= rule.long_len;
        if (r == n || is_long) {
            if (r > run) {
                short_runs.emplace_back(run, r);
                n_short += r - run;
                short_bytes += ho[r] - ho[run];
            }
            run = r + 1;
            if (is_long) longs.push_back(r);
        }
    }
    const bool compact = short_runs.size() > kMaxShortRuns;

    // every locus' ranges and runs, in one pinned array sent once
    std::vector<MlstChunkRun> runs;
    std::vector<ChunkRange> ranges;
    std::vector<size_t> locus_end(n_loci);
    for (uint32_t l = 0; l < n_loci; ++l) {
        cut_chunk_ranges(longs, ho, width[l], k, rule, row_cap, std::max<uint64_t>(ws, 1), &runs, &ranges);
        locus_end[l] = ranges.size();
    }
    uint64_t max_nc = 0, max_bytes = 0, max_runs = 0;
    for (const ChunkRange& g : ranges) {
        max_nc = std::max(max_nc, g.nc);
        max_bytes = std::max(max_bytes, g.bytes);
        max_runs = std::max(max_runs, g.n_runs);
    }

    if (int rc = ws_enter(b0, s)) return rc;
    const uint64_t short_per = std::min(row_cap, std::max<uint64_t>(n_short, 1));
    if (int rc = b0->hits.ensure(std::max(short_per, max_nc) * dmax * 4)) return rc;
    if (int rc = b0->best.ensure(n * L * 4 * 3)) return rc;
    uint32_t* d_rows = b0->hits.as<uint32_t>();
    uint32_t* d_top = b0->best.as<uint32_t>();
    uint32_t* d_score = d_top + n * L;
    uint32_t* d_tied = out.n_tied ? d_score + n * L : nullptr;
    uint64_t* d_nk = nullptr;
    if (out.num_kmers) {  // of every record, long ones too, from the lengths alone
        if (int rc = b0->nk.ensure(n * 8)) return rc;
        if (int rc = b0->nseg.ensure((n + 1) * 8)) return rc;
        d_nk = b0->nk.as<uint64_t>();
        HIPCHK(launch_units(all.offs, n, k, step, d_nk, b0->nseg.as<uint64_t>(), s));
    }

    // ---- short records
    if (!compact) {
        for (const auto& run : short_runs) {
            const uint64_t o = run.first * L;
            if (int rc = mlst_type_span(loci, n_loci, all, ho, run.first, run.second - run.first, row_cap, step, d_rows,
                                        d_top + o, d_score + o, d_tied ? d_tied + o : nullptr, s))
                return rc;
        }
    } else {
        const uint64_t m = n_short;
        if (m >= (1ull << 32)) return fail(XS_ERR_ARG, "at most 2^32-1 short records per call");
        if (int rc = b0->mc_idx_h.ensure((m + 1) * 8 + m * 4)) return rc;
        if (int rc = b0->mc_idx.ensure((m + 1) * 8 + m * 4)) return rc;
        if (int rc = b0->mc_short.ensure(short_bytes + kPad)) return rc;
        if (int rc = b0->mc_out.ensure(m * L * 4 * 3)) return rc;
        uint64_t* co = static_cast<uint64_t*>(b0->mc_idx_h.p);  // the compacted reads' m + 1 offsets, then their indices
        uint32_t* ci = reinterpret_cast<uint32_t*>(co + m + 1);
        uint64_t j = 0, ob = 0;
        for (const auto& run : short_runs)
            for (uint64_t r = run.first; r < run.second; ++r, ++j) {
                co[j] = ob;
                ci[j] = (uint32_t)r;
                ob += ho[r + 1] - ho[r];
            }
        co[m] = ob;
        HIPCHK(hipMemcpyAsync(b0->mc_idx.p, co, (m + 1) * 8 + m * 4, hipMemcpyHostToDevice, s));
        const uint64_t* d_co = b0->mc_idx.as<uint64_t>();
        const uint32_t* d_ci = reinterpret_cast<const uint32_t*>(d_co + m + 1);
        HIPCHK(launch_gather_reads(all.seqs, all.offs, d_ci, m, b0->mc_short.as<uint8_t>(), d_co, s));
        HIPCHK(hipMemsetAsync(b0->mc_short.as<uint8_t>() + short_bytes, 0, kPad, s));
        uint32_t* c_top = b0->mc_out.as<uint32_t>();
        uint32_t* c_score = c_top + m * L;
        uint32_t* c_tied = d_tied ? c_score + m * L : nullptr;
        const Inputs shorts{b0->mc_short.as<uint8_t>(), short_bytes, d_co, m};
        if (int rc = mlst_type_span(loci, n_loci, shorts, co, 0, m, row_cap, step, d_rows, c_top, c_score, c_tied, s))
            return rc;
        HIPCHK(launch_mlst_scatter_rows(d_ci, m, L, c_top, c_score, c_tied, d_top, d_score, d_tied, s));
    }

    // ---- long records
    if (!ranges.empty()) {
        const size_t run_bytes = runs.size() * sizeof(MlstChunkRun);
        if (int rc = b0->mc_runs_h.ensure(run_bytes)) return rc;
        if (int rc = b0->mc_runs.ensure(run_bytes)) return rc;
        if (int rc = b0->mc_text.ensure(max_bytes + kPad)) return rc;
        if (int rc = b0->mc_offs.ensure((max_nc + 1) * 8)) return rc;
        if (int rc = b0->mc_sum.ensure(max_runs * dmax * 8)) return rc;
        if (int rc = b0->mc_key.ensure(max_runs * dmax * 8)) return rc;
        memcpy(b0->mc_runs_h.p, runs.data(), run_bytes);
        HIPCHK(hipMemcpyAsync(b0->mc_runs.p, b0->mc_runs_h.p, run_bytes, hipMemcpyHostToDevice, s));
        uint8_t* text = b0->mc_text.as<uint8_t>();
        uint64_t* coffs = b0->mc_offs.as<uint64_t>();
        auto* sum = b0->mc_sum.as<unsigned long long>();
        auto* key = b0->mc_key.as<unsigned long long>();
        size_t gi = 0;
        for (uint32_t l = 0; l < n_loci; ++l) {
            const uint64_t D = loci[l]->D;
            for (; gi < locus_end[l]; ++gi) {
                const ChunkRange& g = ranges[gi];
                const MlstChunkRun* d_runs = b0->mc_runs.as<MlstChunkRun>() + g.run0;
                const uint64_t keep = g.carry_in ? 1 : 0;  // slot 0 holds the record the last range left unfinished
                if (g.n_runs > keep) {
                    HIPCHK(hipMemsetAsync(sum + keep * D, 0, (g.n_runs - keep) * D * 8, s));
                    HIPCHK(hipMemsetAsync(key + keep * D, 0xFF, (g.n_runs - keep) * D * 8, s));
                }
                HIPCHK(launch_mlst_split(all.seqs, d_runs, g.n_runs, g.nc, k, text, coffs, s));
                const Inputs in{text, g.bytes, coffs, g.nc, g.bytes};
                if (int rc = run_query(loci[l], in, step, d_rows, nullptr, nullptr, s)) return rc;
                HIPCHK(launch_mlst_chunk_acc(d_rows, g.nc, D, &d_runs->row0, kMlstRunWords, g.n_runs, rule.threshold,
                                             g.chunk_base, sum, key, s));
                const uint64_t done = g.n_runs - (g.carry_out ? 1 : 0);
                HIPCHK(launch_mlst_owner_top(sum, key, done, D, &d_runs->rec, kMlstRunWords, d_top + l, d_score + l,
                                             d_tied ? d_tied + l : nullptr, L, s));
                if (g.carry_out && done > 0) {
                    HIPCHK(hipMemcpyAsync(sum, sum + done * D, D * 8, hipMemcpyDeviceToDevice, s));
                    HIPCHK(hipMemcpyAsync(key, key + done * D, D * 8, hipMemcpyDeviceToDevice, s));
                }
            }
        }
    }
    if (int rc = ws_leave(b0, s)) return rc;
    const D2hPart parts[4] = {{out.top, d_top, n * L * 4},
                              {out.top_score, d_score, n * L * 4},
                              {out.n_tied, d_tied, d_tied ? n * L * 4 : 0},
                              {out.num_kmers, d_nk, d_nk ? n * 8 : 0}};
    return d2h_parts(b0, parts, 4, s);
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
        if (int rc = stage_host_reads(b, seqs, offsets, n_rec, &in)) return rc;
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
        if (hit_bytes != 1 && hit_bytes != 2 && hit_bytes != 4) return fail(XS_ERR_ARG, "hit_bytes must be 1, 2 or 4");
        if (step == 0) return fail(XS_ERR_ARG, "step must be >= 1");
        const uint64_t max_nk = max_len >= b->k ? (max_len - b->k) / step + 1 : 0;
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
                for (uint64_t r = 0; r < n; ++r) {  // best_doc_kernel's rule: a unique maximum, else ambiguous
                    const uint32_t* row = rows.data() + r * cols;
                    uint32_t m = 0, arg = 0, cnt = 0;
                    for (uint64_t c = 0; c < cols; ++c) {
                        if (cnt == 0 || row[c] > m) {
                            m = row[c];
                            arg = (uint32_t)c;
                            cnt = 1;
                        } else if (row[c] == m) {
                            ++cnt;
                        }
                    }
                    best_doc[r] = cnt == 1 ? arg : kBestAmbiguous;
                    if (best_hits) best_hits[r] = m;
                }
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
        if (n_direct && direct_hits)
            if (int rc = d2h_pageable(b, direct_hits, d_hits, n_direct * D * 4, b->stream)) return rc;
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
        LociLock lk(loci, n_loci);
        HIPCHK(hipSetDevice(loci[0]->device));
        if (n == 0) return XS_OK;
        DrainStream drain{loci[0]->stream};
        if (int rc = ws_enter(loci[0], loci[0]->stream)) return rc;
        Inputs in;
        if (int rc = upload_reads(loci[0], seqs, offsets, n, loci[0]->stream, &in)) return rc;
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
        LociLock lk(loci, n_loci);
        HIPCHK(hipSetDevice(loci[0]->device));
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
        if (!offsets || (!seqs && n)) return fail(XS_ERR_ARG, "null argument");
        xs_mlst_chunk_rule_t r;
        if (int rc = mlst_contigs_check(loci, n_loci, locus_width, rule, offsets[n] - offsets[0], n, step, out, &r))
            return rc;
        LociLock lk(loci, n_loci);
        HIPCHK(hipSetDevice(loci[0]->device));
        if (n == 0) return XS_OK;
        DrainStream drain{loci[0]->stream};
        if (int rc = ws_enter(loci[0], loci[0]->stream)) return rc;
        Inputs in;
        if (int rc = upload_reads(loci[0], seqs, offsets, n, loci[0]->stream, &in)) return rc;
        return mlst_contigs_run(loci, n_loci, locus_width, r, in, static_cast<const uint64_t*>(loci[0]->offs_h.p), step,
                                workspace_bytes, out);
    });
}

int xs_mlst_type_contigs_device(xs_bank* const* loci, uint32_t n_loci, const uint64_t* locus_width,
                                const xs_mlst_chunk_rule_t* rule, const void* d_seqs, uint64_t seq_bytes,
                                const uint64_t* d_offsets, const uint64_t* host_offsets, uint64_t n, uint32_t step,
                                uint64_t workspace_bytes, uint32_t* top, uint32_t* top_score, uint32_t* n_tied,
                                uint64_t* num_kmers_out) {
    return xs::guard([&]() -> int {
        const MlstTypeOut out{top, top_score, n_tied, num_kmers_out};
        if (n && (!d_seqs || !d_offsets)) return fail(XS_ERR_ARG, "null argument");
        xs_mlst_chunk_rule_t r;
        if (int rc = mlst_contigs_check(loci, n_loci, locus_width, rule, seq_bytes, n, step, out, &r)) return rc;
        LociLock lk(loci, n_loci);
        HIPCHK(hipSetDevice(loci[0]->device));
        if (n == 0) return XS_OK;
        DrainStream drain{loci[0]->stream};
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
    });
}

int xs_mlst_split_size(const uint64_t* lengths, uint64_t n_long, uint64_t width, uint32_t k,
                       const xs_mlst_chunk_rule_t* rule, uint64_t* n_chunks, uint64_t* chunk_bytes) {
    return xs::guard([&]() -> int {
        if ((!lengths && n_long) || !n_chunks || !chunk_bytes) return fail(XS_ERR_ARG, "null argument");
        xs_mlst_chunk_rule_t r;
        if (int rc = chunk_rule_check(rule, &r)) return rc;
        if (k == 0 || width < k) return fail(XS_ERR_ARG, "width must be >= k >= 1");
        if (r.long_len < k) return fail(XS_ERR_ARG, "long_len must be >= k = %u", k);
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
        if (int rc = chunk_rule_check(rule, &r)) return rc;
        if (k == 0 || width < k) return fail(XS_ERR_ARG, "width must be >= k >= 1");
        if (r.long_len < k) return fail(XS_ERR_ARG, "long_len must be >= k = %u", k);
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
        // the accumulators live for this call only: it returns once the outputs are written
        DevBuf acc;
        const uint64_t cells = n_owners * num_docs;
        if (int rc = acc.ensure(cells * 16)) return rc;
        auto* sum = acc.as<unsigned long long>();
        auto* key = sum + cells;
        HIPCHK(hipMemsetAsync(sum, 0, cells * 8, s));
        HIPCHK(hipMemsetAsync(key, 0xFF, cells * 8, s));
        HIPCHK(launch_mlst_chunk_acc(d_hits, n_chunks, num_docs, d_owner_begin, 1, n_owners, threshold, 0, sum, key, s));
        HIPCHK(launch_mlst_owner_top(sum, key, n_owners, num_docs, nullptr, 0, d_top, d_top_score, d_n_tied, out_stride,
                                     s));
        HIPCHK(hipStreamSynchronize(s));
        return XS_OK;
    });
}

}  // extern "C"
