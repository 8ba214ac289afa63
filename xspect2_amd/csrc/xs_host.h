// xs_host.h — what xs_api.cpp, xs_bank_io.cpp, xs_query.cpp and xs_mlst.cpp share: error reporting, the device
// and pinned buffers, the bank handle and its workspace ordering.  Host only: never included
// from a .hip file, and not part of the public ABI.
#pragma once
#include "../../include/xspect_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>

#include "xs_internal.h"

namespace xs {

#define HIPCHK(expr)                                                                           \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return xs::fail(XS_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                            __FILE__, __LINE__);                                               \
    } while (0)

constexpr uint64_t kPad = 64;  // spare bytes after staged host reads

// Host threads of the library's parallel copies and passes: up to 8.
inline int host_threads() {
    static const int n = (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    return n;
}

// fn(t, a, e) over the ranges of [0, n) of up to `threads` threads, t the range's index; one
// range, on the caller's thread, below `serial` items
template <class F>
void par_ranges(uint64_t n, uint64_t serial, int threads, F fn) {
    if (n < serial || threads <= 1) return fn(0, 0, n);
    const uint64_t per = (n + threads - 1) / threads;
    xs::parallel_for(threads, [&](int t) {
        const uint64_t a = per * (uint64_t)t;
        if (a < n) fn(t, a, std::min(n, a + per));
    });
}

// True for page-locked host memory HIP knows (a DMA can take it as it is).
inline bool is_pinned_host(const void* p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) == hipSuccess) return attr.type == hipMemoryTypeHost;
    (void)hipGetLastError();  // pageable memory is "not a HIP pointer"
    return false;
}

// Device bytes a handle's workspace holds now and has held at most at once
// (xs_bank_workspace_bytes).
struct WsAcct {
    uint64_t held = 0, peak = 0;
};

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    WsAcct* acct = nullptr;  // the owning handle's workspace tally, if any
    // Workspace buffers of a bank handle: every enqueue that touches them ends
    // with a record of the handle's ws_ev (ws_leave), so waiting for that event
    // is enough before freeing the old buffer on growth.  Buffers without a
    // guard wait for the device.
    const hipEvent_t* guard_ev = nullptr;
    const bool* guard_used = nullptr;
    int ensure(size_t bytes) {
        if (bytes <= cap && p) return XS_OK;
        if (p) {
            // Growth only: work queued earlier on any stream (a device query on
            // the caller's stream) may still read the old buffer.
            if (guard_ev) {
                if (*guard_used) (void)hipEventSynchronize(*guard_ev);
            } else {
                (void)hipDeviceSynchronize();
            }
            (void)hipFree(p);
            if (acct) acct->held -= cap;
        }
        p = nullptr;
        cap = 0;
        size_t want = bytes < 256 ? 256 : bytes;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess)
            return fail(XS_ERR_HIP, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        cap = want;
        if (acct) acct->peak = std::max(acct->peak, acct->held += want);
        return XS_OK;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
    // give the memory back now (the caller has synchronised every stream that used it)
    void release() {
        if (p) (void)hipFree(p);
        if (acct) acct->held -= cap;
        p = nullptr;
        cap = 0;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

// Pinned host staging for large device -> pageable-host copies.
struct PinnedBuf {
    void* p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap && p) return XS_OK;
        pinned_free(p);
        p = nullptr;
        cap = 0;
        if (int rc = pinned_alloc(bytes, &p)) return rc;
        cap = bytes;
        return XS_OK;
    }
    ~PinnedBuf() { pinned_free(p); }
};

}  // namespace xs

struct xs_bank {
    int kind = 0;
    int device = 0;
    uint32_t k = 0, h = 0, canonicalize = 1;
    uint64_t D = 0, G = 0, page = 0;
    std::vector<uint64_t> sig;
    std::vector<std::string> names;
    // device image
    uint64_t pitch = 0;  // COBS: padded bytes per row
    uint64_t dev_bytes = 0;
    uint64_t nbytes = 0;  // rbloom filter bytes
    xs::WsAcct ws_acct;   // the workspace buffers below (not the image)
    xs::DevBuf image;
    xs::DevBuf groups;
    hipStream_t stream = nullptr;
    std::mutex mu;
    // workspace
    xs::DevBuf seqs, offs, nseg, unit_ofs, unit_read, n_units, scan_tmp, nk, hits, partials, totals, tmp,
        best, narrow, ovf;
    xs::DevBuf rows_read;           // profiling: filter words the rbloom probe loaded
    xs::DevBuf pk_nkc, pk_kofs, pk_scan, pk_entries, pk_tbl, pk_miss, pk_aux;  // partitioned probes (rbloom, COBS)
    // rbloom path choice: member fraction of the last query whose totals have
    // landed (members, k-mers), copied back asynchronously after every query
    xs::DevBuf bloom_tot;
    xs::PinnedBuf bloom_tot_h;
    hipEvent_t bloom_ev = nullptr;
    bool bloom_pending = false;
    double member_frac = 1.0;
    int last_path = XS_PATH_GATHER;
    const char* last_kernel = "";    // name of the probe kernel the last query launched (a string literal)
    xs::ProbeOptions opt;           // path selection (xs_bank_set_probe_options)
    xs::PinnedBuf stage[3];         // D2H staging ring for large host outputs (d2h_parts: 2, HitSink: 3)
    hipEvent_t stage_ev[3] = {nullptr, nullptr, nullptr};
    xs::PinnedBuf hstage[2];        // H2D staging ring for host read batches
    xs::PinnedBuf small_h;          // small host calls: the whole request and its results (query_small)
    xs::PinnedBuf cut_ofs;          // device-read batches: read offsets at the chunk cuts
    xs::PinnedBuf offs_h;           // host batches: the read offsets rebased to 0, for their H2D copy
    xs::DevBuf small_d;
    // MLST typing of contigs (mlst_contigs_run in xs_mlst.cpp): a range's chunk texts, their offsets and
    // accumulators, the call's chunk runs, and for a batch of many short runs the compacted short reads with
    // their index and outputs; a ranked call's n x loci x N rank arrays
    xs::DevBuf mc_text, mc_offs, mc_sum, mc_key, mc_runs, mc_short, mc_idx, mc_out, mc_ranks;
    xs::PinnedBuf mc_runs_h, mc_idx_h;
    hipEvent_t hstage_ev[2] = {nullptr, nullptr};
    hipStream_t copy_stream = nullptr, d2h_stream = nullptr;
    std::vector<hipEvent_t> chunk_ev;  // probe of batch chunk i done
    // The workspace above is shared by every query and build on the handle.  A
    // call enqueued on a different stream than the previous one waits for that
    // one's work on the device (ws_ev), so callers may mix streams freely.
    hipEvent_t ws_ev = nullptr;
    hipStream_t ws_stream = nullptr;
    bool ws_used = false;
    bool profiling = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;  // one pair per profiled probe
    size_t events_used = 0;
    std::vector<hipEvent_t> pass_ev;  // profiling: pass boundaries of the partitioned probes
    std::vector<int> pass_tag;
    size_t pass_used = 0;

    xs_bank(int device_, int kind_) : kind(kind_), device(device_) {
        for (xs::DevBuf* d : {&seqs, &offs, &nseg, &unit_ofs, &unit_read, &n_units, &scan_tmp, &nk, &hits, &partials,
                              &totals, &tmp, &best, &narrow, &ovf, &rows_read, &pk_nkc, &pk_kofs, &pk_scan, &pk_entries,
                              &pk_tbl, &pk_miss, &pk_aux, &bloom_tot, &mc_text, &mc_offs, &mc_sum, &mc_key, &mc_runs,
                              &mc_short, &mc_idx, &mc_out, &mc_ranks}) {
            d->guard_ev = &ws_ev;
            d->guard_used = &ws_used;
            d->acct = &ws_acct;
        }
        small_d.acct = &ws_acct;
    }
    // drains and destroys the handle's streams and events (xs_api.cpp); also the way out of a failed open
    ~xs_bank();

    // hit columns of a query: one per document, one for an rbloom filter (totals carry one more, the k-mers)
    uint64_t cols() const { return kind == XS_BANK_RBLOOM ? 1 : D; }
    uint64_t sig_total() const {
        uint64_t s = 0;
        for (auto v : sig) s += v;
        return s;
    }
    uint64_t payload_bytes() const {
        return kind == XS_BANK_RBLOOM ? nbytes : sig_total() * page;
    }
    xs::CobsView cobs_view() const {
        xs::CobsView v;
        v.rows = image.as<uint8_t>();
        v.groups = groups.as<xs::GroupDesc>();
        v.G = (uint32_t)G;
        v.pitch = (uint32_t)pitch;
        v.nchunks = (uint32_t)((page + 15) / 16);  // chunks that hold doc bits
        v.h = h;
        v.page = page;
        v.D = D;
        v.sig0 = sig.empty() ? 0 : sig[0];
        v.sig_max = 0;
        for (auto x : sig) v.sig_max = x > v.sig_max ? x : v.sig_max;
        return v;
    }
    xs::BloomView bloom_view() const {
        xs::BloomView v;
        v.bits = image.as<uint32_t>();
        v.mbits = nbytes * 8;
        v.magic = xs::barrett_magic(v.mbits);
        v.K = h;
        v.rows_read = profiling ? rows_read.as<uint64_t>() : nullptr;
        return v;
    }
};

namespace xs {

// Order the handle's next enqueue on stream s after its previous one.
inline int ws_enter(xs_bank* b, hipStream_t s) {
    if (b->ws_used && b->ws_stream != s) HIPCHK(hipStreamWaitEvent(s, b->ws_ev, 0));
    return XS_OK;
}
inline int ws_leave(xs_bank* b, hipStream_t s) {
    if (!b->ws_ev) HIPCHK(hipEventCreateWithFlags(&b->ws_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(b->ws_ev, s));
    b->ws_stream = s;
    b->ws_used = true;
    return XS_OK;
}

}  // namespace xs
