// xs_fastx_devside.cpp — the host side of the reader's device mode
// (xs_fastx_open_device; the mode overview is at the top of xs_fastx.cpp, the
// kernels are in xs_fastx_dev.hip): pooled buffers, the device sides and stream
// sets kept between readers, the pinned ring that carries a window's text to
// HBM with its loader thread, and the record finding on the device.
#include "xs_fastx.h"

#include <hip/hip_runtime.h>

#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <thread>

using namespace xs::fx;

namespace xs::fx {
namespace {

double fx_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Pinned host and device buffers outlive their reader in a process-wide pool:
// pinning host memory costs (xs::pinned_alloc) and a hipFree synchronises
// the device, so a reader per input file would otherwise pay more for its
// buffers than for its parse.  Reuse takes the smallest pooled buffer that
// fits and is at most 4x the request.
struct BufPool {
    struct Entry {
        void* p;
        size_t cap;
        int device;  // -1: pinned host memory
    };
    std::mutex mu;
    std::vector<Entry> free_list;
    size_t bytes = 0;
    static constexpr size_t kMaxBytes = size_t(6) << 30;
    static constexpr size_t kMaxEntries = 96;
    void* take(size_t want, int device, size_t* cap) {
        std::lock_guard<std::mutex> g(mu);
        size_t best = free_list.size();
        for (size_t i = 0; i < free_list.size(); ++i) {
            const Entry& e = free_list[i];
            if (e.device == device && e.cap >= want && e.cap / 4 <= want &&
                (best == free_list.size() || e.cap < free_list[best].cap))
                best = i;
        }
        if (best == free_list.size()) return nullptr;
        void* p = free_list[best].p;
        *cap = free_list[best].cap;
        bytes -= *cap;
        free_list.erase(free_list.begin() + (ptrdiff_t)best);
        return p;
    }
    bool give(void* p, size_t cap, int device) {  // false: the caller frees it
        std::lock_guard<std::mutex> g(mu);
        if (bytes + cap > kMaxBytes || free_list.size() >= kMaxEntries) return false;
        free_list.push_back({p, cap, device});
        bytes += cap;
        return true;
    }
};
BufPool g_pool;

// A grow-only buffer out of g_pool (contents are not preserved): pinned host
// memory, pooled as device -1, or memory of the device that is current when
// it allocates.  Every way into the device mode sets the reader's device
// first and hipMalloc allocates there, so the pool's key is the memory's
// device without anybody having to tell the buffer.
template <bool kPinned>
struct PoolBuf {
    void* p = nullptr;
    size_t cap = 0;
    int device = -1;
    // exact: no 1/8 headroom (a fixed-size buffer)
    int ensure(size_t bytes, bool exact = false) {
        if (bytes <= cap && p) return XS_OK;
        release();
        if (!kPinned && hipGetDevice(&device) != hipSuccess)
            return xs::set_error(XS_ERR_HIP, "no current device for the device reader");
        if ((p = g_pool.take(bytes, device, &cap))) return XS_OK;
        const size_t want = std::max<size_t>(exact ? bytes : bytes + bytes / 8, kPinned ? 1 << 16 : 4096);
        const double t0 = fx_ms();
        if (kPinned ? xs::pinned_alloc(want, &p) != XS_OK : hipMalloc(&p, want) != hipSuccess) {
            p = nullptr;
            return xs::set_error(XS_ERR_HIP, kPinned ? "pinned allocation failed for the device reader"
                                                     : "hipMalloc failed for the device reader");
        }
        if (kPinned && fx_trace()) fprintf(stderr, "[fastx-device] pinned %zu B in %.2f ms\n", want, fx_ms() - t0);
        cap = want;
        return XS_OK;
    }
    void release() {
        if (p && !g_pool.give(p, cap, device)) {
            if (fx_trace())
                fprintf(stderr, kPinned ? "[fastx-device] unpinned %zu B\n" : "[fastx-device] hipFree %zu B\n", cap);
            if (kPinned) xs::pinned_free(p);
            else (void)hipFree(p);
        }
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
    PoolBuf() = default;
    PoolBuf(const PoolBuf&) = delete;
    PoolBuf& operator=(const PoolBuf&) = delete;
    ~PoolBuf() { release(); }
};
using PinBuf = PoolBuf<true>;
using DBuf = PoolBuf<false>;

constexpr size_t kPieceBytes = 4u << 20;  // pread + DMA unit of a window's text
// pread threads of a window load: 6 outrun the DMA (~50 GB/s) and leave the
// caller's threads their CPU share (profiles/r04_e2e_ring.txt)
constexpr size_t kLoadThreads = 6;
constexpr size_t kDevPad = 64;            // defined zero bytes past a batch's sequences

// The streams and events of a device side.  Those of closed readers are kept
// for the next reader on the same device: creating them costs about a
// millisecond per open, as much as parsing the first window.
struct StreamSet {
    int device = 0;
    hipStream_t stream = nullptr;  // parse kernels
    hipStream_t copy = nullptr;    // text DMA
    // Window text in two slots: the next window loads into one while the
    // current one is parsed from the other.
    hipEvent_t text_ev[2] = {nullptr, nullptr};
    hipEvent_t kern_ev = nullptr;                // a batch's device data complete
    hipEvent_t host_ev[2] = {nullptr, nullptr};  // slot s's host arrays complete
    template <class F>
    void each_event(F f) {
        for (hipEvent_t* e : {&text_ev[0], &text_ev[1], &kern_ev, &host_ev[0], &host_ev[1]}) f(*e);
    }
};
std::mutex g_ss_mu;
std::vector<StreamSet> g_ss;
constexpr size_t kStreamSetsKept = 16;

bool take_streams(StreamSet& ss) {  // a kept set of ss.device
    std::lock_guard<std::mutex> g(g_ss_mu);
    for (size_t i = 0; i < g_ss.size(); ++i) {
        if (g_ss[i].device != ss.device) continue;
        ss = g_ss[i];
        g_ss.erase(g_ss.begin() + (long)i);
        return true;
    }
    return false;
}

}  // namespace

struct DevSide {
    StreamSet ss;
    // Window text goes to HBM through a ring of pinned pieces (ring_pieces()
    // x kPieceBytes): pinning cost ~0.19 ms per MiB with hipHostMalloc (~0.02
    // with xs::pinned_alloc's registered 2 MiB pages), and whole-window pinned
    // buffers (two of up to 288 MiB) are more than a window needs at once; the
    // ring is 128 MiB whatever the window.
    PinBuf ring;
    PinBuf pin[2];                     // XSPECT2_AMD_FX_RING=0: a window's whole text per slot
    hipEvent_t ring_ev[kRingMax] = {};  // the DMA out of ring piece r done (recorded on ss.copy)
    bool ring_used[kRingMax] = {};
    PinBuf status;      // small D2H results
    DBuf text[2];       // a window's text, zero-padded to whole tiles
    DBuf tiles, tile_ofs, nl, temp, flag;
    DBuf hdr, hofs, line_src, line_len, line_ofs, rec_line, lens, maxlen;
    DBuf seq_src, seq_len, id_src, id_len, desc_src, desc_len, id_ofs, desc_ofs, ids_d, descs_d;
    DBuf seqs[2], offs[2];
    DBuf fq_blk, fq_blk_ofs, fq_status;  // FASTQ record blocks' sums and offsets, the window's status
    PinBuf ids[2], id_offs[2], descs[2], desc_offs[2], hoffs[2];
    int flip = 0;
    // Text of the next windows, loaded in order by `loader` while the caller
    // works: up to two ahead, window j+2 into window j's slot as soon as j is
    // parsed (the parse is the only reader of a slot's text).
    struct PfJob {
        size_t lo, hi;
        int slot;
        bool started, done;
        int rc;
        std::string err;
    };
    std::thread loader;
    std::mutex pf_mu;
    std::condition_variable pf_cv;
    std::deque<PfJob> pf_q;  // oldest first; popped by text_for once done
    bool pf_stop = false;
    int next_text = 0;  // text slot of the next window queued or loaded inline
    double load_ms[2] = {0, 0};  // each slot's last load_text: pread + DMA queueing
    ~DevSide();
};

namespace {

// End the loader thread after the loads it has started (a queued load
// that has not started is dropped), and forget the queue.
void stop_loader(DevSide& d) {
    {
        std::lock_guard<std::mutex> g(d.pf_mu);
        d.pf_stop = true;
    }
    d.pf_cv.notify_all();
    if (d.loader.joinable()) d.loader.join();
    d.pf_stop = false;
    d.pf_q.clear();
}

// Whole device sides of closed readers, kept for the next reader on the same
// device: their streams, events and buffers at the sizes the last file grew
// them to, so a process reading file after file allocates and pins nothing
// after its first (a reader's buffers otherwise went back to g_pool piece by
// piece and the next reader's ramp took them out in a different order,
// pinning and freeing afresh: 17 -> 26 ms per 313 MB file over six files,
// profiles/r04_e2e_ring.txt).  A batch's arrays are the reader's and are
// invalid after xs_fastx_close, as before.
std::mutex g_ds_mu;
std::vector<DevSide*> g_ds;
constexpr size_t kDevSidesKept = 4;

DevSide* take_devside(int device) {
    std::lock_guard<std::mutex> g(g_ds_mu);
    for (size_t i = 0; i < g_ds.size(); ++i) {
        if (g_ds[i]->ss.device != device) continue;
        DevSide* d = g_ds[i];
        g_ds.erase(g_ds.begin() + (long)i);
        return d;
    }
    return nullptr;
}

// Quiesce a closed reader's device side and keep it (or destroy it when
// kDevSidesKept are kept already or its streams were never made).
void put_devside(DevSide* d) {
    if (!d) return;
    stop_loader(*d);
    const StreamSet& ss = d->ss;
    bool ok = ss.stream && ss.copy && hipSetDevice(ss.device) == hipSuccess &&
              hipStreamSynchronize(ss.stream) == hipSuccess && hipStreamSynchronize(ss.copy) == hipSuccess;
    if (ok) {
        d->flip = 0;
        d->next_text = 0;
        d->load_ms[0] = d->load_ms[1] = 0;
        std::lock_guard<std::mutex> g(g_ds_mu);
        if (g_ds.size() < kDevSidesKept) {
            g_ds.push_back(d);
            return;
        }
    }
    delete d;
}

}  // namespace

DevSide::~DevSide() {
    stop_loader(*this);
    (void)hipSetDevice(ss.device);
    if (ss.stream) (void)hipStreamSynchronize(ss.stream);
    if (ss.copy) (void)hipStreamSynchronize(ss.copy);
    for (hipEvent_t e : ring_ev)
        if (e) (void)hipEventDestroy(e);
    bool all = ss.stream && ss.copy;
    ss.each_event([&](hipEvent_t& e) { all = all && e; });
    if (all) {
        std::lock_guard<std::mutex> g(g_ss_mu);
        if (g_ss.size() < kStreamSetsKept) {
            g_ss.push_back(ss);
            return;
        }
    }
    ss.each_event([](hipEvent_t& e) {
        if (e) (void)hipEventDestroy(e);
    });
    if (ss.stream) (void)hipStreamDestroy(ss.stream);
    if (ss.copy) (void)hipStreamDestroy(ss.copy);
}

namespace {

struct FxTimes {
    double count = 0, records = 0, copy = 0;
};
thread_local FxTimes g_fx;

#define FXCHK(expr)                                                                                     \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) return xs::set_error(XS_ERR_HIP, hipGetErrorString(_e));                 \
    } while (0)

// What the pread workers of a window load and the thread that queues the
// pieces' DMAs share.
struct PieceState {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<uint8_t> done;  // piece p is in its host buffer
    size_t queued = 0;          // pieces whose DMA is queued (in order)
    bool failed = false;
    void fail() {
        {
            std::lock_guard<std::mutex> g(mu);
            failed = true;
        }
        cv.notify_all();
    }
};

bool pread_piece(int fd, char* dst, size_t n, size_t off) {
    for (size_t o = 0; o < n;) {
        const ssize_t got = pread(fd, dst + o, n - o, (off_t)(off + o));
        if (got <= 0) {
            if (got < 0 && errno == EINTR) continue;
            return false;
        }
        o += (size_t)got;
    }
    return true;
}

// The text of [lo, hi) (file offsets) into d.text[ts] (zero-padded to whole
// tiles), through the pinned ring: host threads pread 4 MiB pieces into ring
// slots, the DMA of each piece is queued on the copy stream as soon as it is
// in, and a ring slot is reused once its previous DMA has completed.
// d.ss.text_ev[ts] marks the end.
int load_text(xs_fastx* r, size_t lo, size_t hi, int ts) {
    DevSide& d = *r->dev;
    const double t0 = fx_ms();
    FXCHK(hipSetDevice(d.ss.device));
    const size_t span = hi - lo;
    const size_t tiles = std::max<size_t>(1, (span + xs::kFxTile - 1) / xs::kFxTile);
    const size_t padded = tiles * xs::kFxTile;
    DBuf& text = d.text[ts];
    const size_t R = ring_pieces();
    if (R) {
        if (int rc = d.ring.ensure(R * kPieceBytes, true)) return rc;
        for (size_t i = 0; i < R; ++i)
            if (!d.ring_ev[i]) FXCHK(hipEventCreateWithFlags(&d.ring_ev[i], hipEventDisableTiming));
    } else if (int rc = d.pin[ts].ensure(span + 1)) {
        return rc;
    }
    char* const host = R ? d.ring.as<char>() : d.pin[ts].as<char>();
    // host buffer of piece p: its ring slot, or its place in the window's buffer
    auto at = [&](size_t p) { return host + (R ? p % R : p) * kPieceBytes; };
    if (int rc = text.ensure(padded + 16)) return rc;
    const size_t pieces = (span + kPieceBytes - 1) / kPieceBytes;
    // pread outruns the DMA (~50 GB/s) with a few threads; more only burn the
    // CPU share the caller's own threads need
    const int T = (int)std::max<size_t>(1, std::min<size_t>({(size_t)r->threads, kLoadThreads, pieces}));
    PieceState st;
    st.done.assign(pieces, 0);
    auto work = [&](int t) {
        for (size_t p = (size_t)t; p < pieces; p += (size_t)T) {
            bool bad = false;
            if (R) {
                const size_t slot = p % R;
                {   // the ring slot's previous piece must be on its way before it is overwritten
                    std::unique_lock<std::mutex> g(st.mu);
                    st.cv.wait(g, [&] { return st.failed || p < R || st.queued > p - R; });
                    if (st.failed) return;
                }
                if (d.ring_used[slot] && hipEventSynchronize(d.ring_ev[slot]) != hipSuccess) bad = true;
            }
            const size_t o = p * kPieceBytes, n = std::min(span, o + kPieceBytes) - o;
            if (!bad) bad = !pread_piece(r->fd, at(p), n, lo + o);
            {
                std::lock_guard<std::mutex> g(st.mu);
                st.done[p] = 1;
                st.failed |= bad;
            }
            st.cv.notify_all();
        }
    };
    xs::ThreadGroup th;  // pread workers beside this thread, which queues each piece's DMA
    try {
        for (int t = 0; t < T; ++t) th.start(work, t);
    } catch (...) {  // the workers already started stop at `failed` before the group joins them
        st.fail();
        throw;
    }
    int rc = XS_OK;
    for (size_t p = 0; p < pieces && !rc; ++p) {  // queue each piece's DMA as soon as it is in
        {
            std::unique_lock<std::mutex> g(st.mu);
            st.cv.wait(g, [&] { return st.done[p] != 0 || st.failed; });
            if (st.failed) break;
        }
        const size_t o = p * kPieceBytes, n = std::min(span, o + kPieceBytes) - o;
        hipError_t e = hipMemcpyAsync(text.as<char>() + o, at(p), n, hipMemcpyHostToDevice, d.ss.copy);
        if (e == hipSuccess && R) e = hipEventRecord(d.ring_ev[p % R], d.ss.copy);
        std::lock_guard<std::mutex> g(st.mu);
        if (e != hipSuccess) {
            rc = xs::set_error(XS_ERR_HIP, hipGetErrorString(e));
            st.failed = true;
        } else {
            if (R) d.ring_used[p % R] = true;
            st.queued = p + 1;
        }
        st.cv.notify_all();
    }
    th.join();
    if (rc) return rc;
    if (st.failed) return xs::set_error(XS_ERR_IO, "read failed while loading the window's text");
    FXCHK(hipMemsetAsync(text.as<char>() + span, 0, padded + 16 - span, d.ss.copy));
    FXCHK(hipEventRecord(d.ss.text_ev[ts], d.ss.copy));
    d.load_ms[ts] = fx_ms() - t0;
    return XS_OK;
}

// The loader thread: loads queued windows in order until stopped.
void loader_main(xs_fastx* r) {
    DevSide& d = *r->dev;
    std::unique_lock<std::mutex> g(d.pf_mu);
    for (;;) {
        DevSide::PfJob* job = nullptr;
        d.pf_cv.wait(g, [&] {
            if (d.pf_stop) return true;
            for (auto& j : d.pf_q)
                if (!j.started) {
                    job = &j;  // deque references survive push_back and pop_front of others
                    return true;
                }
            return false;
        });
        if (d.pf_stop) return;
        job->started = true;
        const size_t lo = job->lo, hi = job->hi;
        const int slot = job->slot;
        g.unlock();
        const double t0 = fx_ms();
        const int rc = load_text(r, lo, hi, slot);
        std::string err = rc ? xs_last_error() : "";
        if (fx_trace()) fprintf(stderr, "[fastx-device] t=%.2f prefetch %zu+%zu done in %.2f ms\n", fx_ms(), lo, hi - lo,
                                fx_ms() - t0);
        g.lock();
        job->rc = rc;
        job->err = std::move(err);
        job->done = true;
        d.pf_cv.notify_all();
    }
}

// Queue [lo, hi) for the next text slot (in window order).
void queue_window(xs_fastx* r, size_t lo, size_t hi) {
    DevSide& d = *r->dev;
    {
        std::lock_guard<std::mutex> g(d.pf_mu);
        d.pf_q.push_back(DevSide::PfJob{lo, hi, d.next_text, false, false, XS_OK, std::string()});
        d.next_text ^= 1;
    }
    if (!d.loader.joinable()) d.loader = std::thread(loader_main, r);
    d.pf_cv.notify_all();
}

bool is_queued(DevSide& d, size_t lo) {
    std::lock_guard<std::mutex> g(d.pf_mu);
    for (const auto& j : d.pf_q)
        if (j.lo == lo) return true;
    return false;
}

// Wait for every queued load to finish and forget them.
void drain_loads(DevSide& d) {
    std::unique_lock<std::mutex> g(d.pf_mu);
    d.pf_cv.wait(g, [&] {
        for (const auto& j : d.pf_q)
            if (!j.done && (j.started || !d.pf_stop)) return false;
        return true;
    });
    d.pf_q.clear();
}

// Wait for the text of [lo, hi) to be queued for its slot (loading it now if
// it is not the oldest queued window); *ts = the slot, *prefetched = whether
// it came from the queue.
int text_for(xs_fastx* r, size_t lo, size_t hi, int* ts, bool* prefetched) {
    DevSide& d = *r->dev;
    *prefetched = false;
    {
        std::unique_lock<std::mutex> g(d.pf_mu);
        if (!d.pf_q.empty() && d.pf_q.front().lo == lo && d.pf_q.front().hi == hi) {
            d.pf_cv.wait(g, [&] { return d.pf_q.front().done; });
            DevSide::PfJob j = std::move(d.pf_q.front());
            d.pf_q.pop_front();
            *ts = j.slot;
            *prefetched = true;
            if (j.rc) return xs::set_error(j.rc, j.err.c_str());
            return XS_OK;
        }
    }
    // other windows than the queued ones (the caller changed its batch size):
    // let those loads finish, then load this one here
    drain_loads(d);
    {
        std::lock_guard<std::mutex> g(d.pf_mu);
        *ts = d.next_text;
        d.next_text ^= 1;
    }
    return load_text(r, lo, hi, *ts);
}

// ---- record finding on the device ------------------------------------------
// A window's result words in d.status (pinned), copied back by its record pass.
struct FxStatus {
    uint64_t bad, n, sbytes, ibytes, dbytes, max_len;  // bad: the device rules do not cover the window
};
// A window's text as the steps of its parse see it.
struct FxWindow {
    const uint8_t* text;    // d.text[ts], zero-padded to whole tiles
    uint64_t span, tiles;
    uint64_t newlines, L;   // L: lines, a last one without '\n' included
    bool fasta;
};

// Newlines of the text: per-tile counts and their scan into d.tile_ofs; the
// total comes back with the first of a window's two stream synchronisations.
int count_newlines(DevSide& d, FxWindow& w) {
    const hipStream_t s = d.ss.stream;
    for (DBuf* b : {&d.tiles, &d.tile_ofs})
        if (int rc = b->ensure((w.tiles + 1) * 8)) return rc;
    if (int rc = d.status.ensure(64)) return rc;
    if (int rc = d.flag.ensure(8)) return rc;
    const size_t tb = xs::fx_temp_bytes(w.tiles + 1);
    if (int rc = d.temp.ensure(tb)) return rc;
    FXCHK(xs::launch_fx_count(w.text, w.tiles, d.tiles.as<uint64_t>(), s));
    FXCHK(hipMemsetAsync(d.tiles.as<uint64_t>() + w.tiles, 0, 8, s));
    FXCHK(xs::launch_scan(d.temp.p, tb, d.tiles.as<uint64_t>(), d.tile_ofs.as<uint64_t>(), w.tiles + 1, s));
    const double t0 = fx_ms();
    FXCHK(hipMemcpyAsync(d.status.p, d.tile_ofs.as<uint64_t>() + w.tiles, 8, hipMemcpyDeviceToHost, s));
    FXCHK(hipStreamSynchronize(s));
    g_fx.count = fx_ms() - t0;
    w.newlines = d.status.as<uint64_t>()[0];
    return XS_OK;
}

// FASTA record pass over the window's lines: header lines, each line's run and
// record, the records' offsets, id and title runs, and the status words.
int fasta_records(DevSide& d, const FxWindow& w, size_t tb, const xs::FxRuns& runs, uint64_t* offs) {
    const hipStream_t s = d.ss.stream;
    const uint64_t L = w.L;
    const uint32_t* nl = d.nl.as<uint32_t>();
    FxStatus* st = d.status.as<FxStatus>();
    for (DBuf* b : {&d.hdr, &d.hofs, &d.line_len, &d.line_ofs, &d.lens})
        if (int rc = b->ensure((L + 1) * 8)) return rc;
    for (DBuf* b : {&d.line_src, &d.rec_line})
        if (int rc = b->ensure((L + 1) * 4)) return rc;
    // records past the last header keep zero-length ids and titles
    FXCHK(hipMemsetAsync(d.id_len.p, 0, (L + 1) * 8, s));
    FXCHK(hipMemsetAsync(d.desc_len.p, 0, (L + 1) * 8, s));
    FXCHK(hipMemsetAsync(d.lens.p, 0, (L + 1) * 8, s));
    FXCHK(xs::launch_fa_headers(w.text, nl, L, d.hdr.as<uint64_t>(), s));
    FXCHK(hipMemsetAsync(d.hdr.as<uint64_t>() + L, 0, 8, s));
    FXCHK(xs::launch_scan(d.temp.p, tb, d.hdr.as<uint64_t>(), d.hofs.as<uint64_t>(), L + 1, s));
    FXCHK(xs::launch_fa_lines(w.text, nl, L, d.hofs.as<uint64_t>(), d.line_src.as<uint32_t>(),
                              d.line_len.as<uint64_t>(), d.rec_line.as<uint32_t>(), runs, d.flag.as<uint32_t>(), s));
    FXCHK(hipMemsetAsync(d.line_len.as<uint64_t>() + L, 0, 8, s));
    FXCHK(xs::launch_scan(d.temp.p, tb, d.line_len.as<uint64_t>(), d.line_ofs.as<uint64_t>(), L + 1, s));
    FXCHK(xs::launch_fa_offsets(d.rec_line.as<uint32_t>(), d.line_ofs.as<uint64_t>(), L,
                                d.hofs.as<uint64_t>() + L, offs, d.lens.as<uint64_t>(), s));
    FXCHK(xs::launch_scan(d.temp.p, tb, d.id_len.as<uint64_t>(), d.id_ofs.as<uint64_t>(), L + 1, s));
    FXCHK(xs::launch_scan(d.temp.p, tb, d.desc_len.as<uint64_t>(), d.desc_ofs.as<uint64_t>(), L + 1, s));
    FXCHK(xs::launch_max_u64(d.temp.p, tb, d.lens.as<uint64_t>(), L, d.maxlen.as<uint64_t>(), s));
    FXCHK(hipMemcpyAsync(&st->n, d.hofs.as<uint64_t>() + L, 8, hipMemcpyDeviceToHost, s));
    FXCHK(hipMemcpyAsync(&st->sbytes, d.line_ofs.as<uint64_t>() + L, 8, hipMemcpyDeviceToHost, s));
    FXCHK(hipMemcpyAsync(&st->ibytes, d.id_ofs.as<uint64_t>() + L, 8, hipMemcpyDeviceToHost, s));
    FXCHK(hipMemcpyAsync(&st->dbytes, d.desc_ofs.as<uint64_t>() + L, 8, hipMemcpyDeviceToHost, s));
    st->bad = 0;  // the flag is 32 bits wide
    FXCHK(hipMemcpyAsync(&st->bad, d.flag.p, 4, hipMemcpyDeviceToHost, s));
    FXCHK(hipMemcpyAsync(&st->max_len, d.maxlen.p, 8, hipMemcpyDeviceToHost, s));
    return XS_OK;
}

// FASTQ record pass over n four-line records: the records, their offsets and
// the window's status in three kernels and one copy back.
int fastq_records(DevSide& d, const FxWindow& w, uint64_t n, const xs::FxRuns& runs, uint64_t* offs) {
    const hipStream_t s = d.ss.stream;
    const uint64_t nblk = (n + 255) / 256;
    if (int rc = d.fq_blk.ensure((nblk + 1) * sizeof(xs::FqBlockSums))) return rc;
    if (int rc = d.fq_blk_ofs.ensure((nblk + 1) * 3 * 8)) return rc;
    if (int rc = d.fq_status.ensure(sizeof(FxStatus))) return rc;
    FXCHK(xs::launch_fq_records(w.text, d.nl.as<uint32_t>(), n, runs, d.flag.as<uint32_t>(),
                                static_cast<xs::FqBlockSums*>(d.fq_blk.p), d.fq_blk_ofs.as<uint64_t>(), offs,
                                d.id_ofs.as<uint64_t>(), d.desc_ofs.as<uint64_t>(), d.fq_status.as<uint64_t>(), s));
    FXCHK(hipMemcpyAsync(d.status.p, d.fq_status.p, sizeof(FxStatus), hipMemcpyDeviceToHost, s));
    return XS_OK;
}

// Line starts of the window, then the record runs for its format: where each
// record's sequence, id and title lie in the text, and the status words.
int find_records(DevSide& d, const FxWindow& w, int slot) {
    const hipStream_t s = d.ss.stream;
    const uint64_t nmax = w.fasta ? w.L : w.L / 4;  // records, or an upper bound of them
    if (int rc = d.nl.ensure(w.L * 4 + 4)) return rc;
    const size_t tb = xs::fx_temp_bytes(nmax + 1);
    if (int rc = d.temp.ensure(tb)) return rc;
    FXCHK(xs::launch_fx_positions(w.text, w.tiles, d.tile_ofs.as<uint64_t>(), d.nl.as<uint32_t>(), s));
    if (w.L > w.newlines) FXCHK(hipMemsetD32Async(d.nl.as<uint32_t>() + w.newlines, (int)w.span, 1, s));
    FXCHK(hipMemsetAsync(d.flag.p, 0, 4, s));
    for (DBuf* b : {&d.seq_src, &d.id_src, &d.desc_src})
        if (int rc = b->ensure((nmax + 1) * 4)) return rc;
    for (DBuf* b : {&d.seq_len, &d.id_len, &d.desc_len, &d.id_ofs, &d.desc_ofs})
        if (int rc = b->ensure((nmax + 1) * 8)) return rc;
    if (int rc = d.offs[slot].ensure((nmax + 1) * 8)) return rc;
    if (int rc = d.maxlen.ensure(8)) return rc;
    const xs::FxRuns runs{d.seq_src.as<uint32_t>(), d.seq_len.as<uint64_t>(), d.id_src.as<uint32_t>(),
                          d.id_len.as<uint64_t>(), d.desc_src.as<uint32_t>(), d.desc_len.as<uint64_t>()};
    uint64_t* offs = d.offs[slot].as<uint64_t>();
    return w.fasta ? fasta_records(d, w, tb, runs, offs) : fastq_records(d, w, nmax, runs, offs);
}

// The batch's buffers in slot `slot` for the sizes the status reports.
int size_outputs(DevSide& d, const FxStatus& st, int slot) {
    if (int rc = d.seqs[slot].ensure(st.sbytes + kDevPad)) return rc;
    if (int rc = d.ids_d.ensure(st.ibytes + 1)) return rc;
    if (int rc = d.descs_d.ensure(st.dbytes + 1)) return rc;
    if (int rc = d.ids[slot].ensure(st.ibytes + 1)) return rc;
    if (int rc = d.descs[slot].ensure(st.dbytes + 1)) return rc;
    for (PinBuf* b : {&d.id_offs[slot], &d.desc_offs[slot], &d.hoffs[slot]})
        if (int rc = b->ensure((st.n + 1) * 8)) return rc;
    return XS_OK;
}

// The runs out of the text into the batch: sequences (zero-padded), ids and
// titles.  d.ss.kern_ev marks the batch's device data, what the caller probes.
int copy_runs(DevSide& d, const FxWindow& w, const FxStatus& st, int slot) {
    const hipStream_t s = d.ss.stream;
    uint8_t* seqs = d.seqs[slot].as<uint8_t>();
    if (w.fasta)
        FXCHK(xs::launch_fx_copy(w.text, d.line_src.as<uint32_t>(), d.line_ofs.as<uint64_t>(), w.L, st.sbytes, seqs, s));
    else
        FXCHK(xs::launch_fx_copy(w.text, d.seq_src.as<uint32_t>(), d.offs[slot].as<uint64_t>(), st.n, st.sbytes, seqs, s));
    FXCHK(hipMemsetAsync(seqs + st.sbytes, 0, kDevPad, s));
    FXCHK(xs::launch_fx_copy(w.text, d.id_src.as<uint32_t>(), d.id_ofs.as<uint64_t>(), st.n, st.ibytes,
                             d.ids_d.as<uint8_t>(), s));
    FXCHK(xs::launch_fx_copy(w.text, d.desc_src.as<uint32_t>(), d.desc_ofs.as<uint64_t>(), st.n, st.dbytes,
                             d.descs_d.as<uint8_t>(), s));
    FXCHK(hipEventRecord(d.ss.kern_ev, s));
    return XS_OK;
}

// Ids, titles and offsets to the slot's pinned arrays: they land behind the
// caller's probe; xs_fastx_wait_host waits for them (d.ss.host_ev[slot]).
int queue_host_copies(DevSide& d, const FxStatus& st, int slot) {
    const hipStream_t s = d.ss.stream;
    if (st.ibytes) FXCHK(hipMemcpyAsync(d.ids[slot].p, d.ids_d.p, st.ibytes, hipMemcpyDeviceToHost, s));
    if (st.dbytes) FXCHK(hipMemcpyAsync(d.descs[slot].p, d.descs_d.p, st.dbytes, hipMemcpyDeviceToHost, s));
    FXCHK(hipMemcpyAsync(d.id_offs[slot].p, d.id_ofs.p, (st.n + 1) * 8, hipMemcpyDeviceToHost, s));
    FXCHK(hipMemcpyAsync(d.desc_offs[slot].p, d.desc_ofs.p, (st.n + 1) * 8, hipMemcpyDeviceToHost, s));
    FXCHK(hipMemcpyAsync(d.hoffs[slot].p, d.offs[slot].p, (st.n + 1) * 8, hipMemcpyDeviceToHost, s));
    FXCHK(hipEventRecord(d.ss.host_ev[slot], s));
    return XS_OK;
}

// Record finding on the device for the window [lo, hi) whose text is queued
// for d.text.  *ok = false: the window needs the host parser (nothing of the
// batch is kept).  On success the batch is in slot `slot` and `out` is filled.
int parse_on_device(xs_fastx* r, size_t lo, size_t hi, int slot, int ts, bool* ok, xs_fastx_dbatch* out) {
    DevSide& d = *r->dev;
    *ok = false;
    const size_t span = hi - lo;
    if (span == 0 || span >= (1ull << 31) - xs::kFxTile) {  // u32 positions, int scan sizes: host parser
        // the slot's text DMA must be done before the slot is queued for a later window
        // (whose larger buffer could otherwise take this one's back while it is written)
        FXCHK(hipEventSynchronize(d.ss.text_ev[ts]));
        return XS_OK;
    }
    FXCHK(hipStreamWaitEvent(d.ss.stream, d.ss.text_ev[ts], 0));
    FxWindow w{d.text[ts].as<uint8_t>(), span, (span + xs::kFxTile - 1) / xs::kFxTile, 0, 0,
               r->format == XS_FASTX_FASTA};
    if (int rc = count_newlines(d, w)) return rc;
    const double t1 = fx_ms();
    w.L = w.newlines + (r->base[hi - 1] != '\n' ? 1 : 0);  // a last line without '\n' ends at hi
    if (!w.fasta && (w.L == 0 || w.L % 4)) return XS_OK;
    if (int rc = find_records(d, w, slot)) return rc;
    FXCHK(hipStreamSynchronize(d.ss.stream));
    const double t2 = fx_ms();
    g_fx.records = t2 - t1;
    const FxStatus& st = *d.status.as<FxStatus>();
    if ((uint32_t)st.bad) return XS_OK;
    if (int rc = size_outputs(d, st, slot)) return rc;
    const double t2a = fx_ms();
    if (int rc = copy_runs(d, w, st, slot)) return rc;
    const double t2b = fx_ms();
    if (int rc = queue_host_copies(d, st, slot)) return rc;
    const double t2c = fx_ms();
    FXCHK(hipEventSynchronize(d.ss.kern_ev));
    g_fx.copy = fx_ms() - t2;
    if (fx_trace())
        fprintf(stderr, "[fastx-device] copy phase: buffers %.2f launches %.2f D2H queue %.2f wait %.2f ms\n", t2a - t2,
                t2b - t2a, t2c - t2b, fx_ms() - t2c);
    *ok = true;
    out->host_ready = d.ss.host_ev[slot];
    out->n = st.n;
    out->seq_bytes = st.sbytes;
    out->seqs = d.seqs[slot].as<uint8_t>();
    out->offsets = d.offs[slot].as<uint64_t>();
    out->host_offsets = d.hoffs[slot].as<uint64_t>();
    out->max_len = st.max_len;
    out->ids = d.ids[slot].as<char>();
    out->id_offsets = d.id_offs[slot].as<uint64_t>();
    out->descs = d.descs[slot].as<char>();
    out->desc_offsets = d.desc_offs[slot].as<uint64_t>();
    out->parsed_on_device = 1;
    return XS_OK;
}

// A host batch into device slot `slot` (the host parser's result for a window
// the device rules do not cover, or a wrapped FASTQ file's batch).
int upload_host_batch(xs_fastx* r, const xs_fastx_batch& hb, int slot, xs_fastx_dbatch* out) {
    DevSide& d = *r->dev;
    const hipStream_t s = d.ss.stream;
    if (int rc = d.seqs[slot].ensure(hb.seq_bytes + kDevPad)) return rc;
    if (int rc = d.offs[slot].ensure((hb.n + 1) * 8)) return rc;
    uint8_t* seqs = d.seqs[slot].as<uint8_t>();
    if (hb.seq_bytes) FXCHK(hipMemcpyAsync(seqs, hb.seqs, hb.seq_bytes, hipMemcpyHostToDevice, s));
    FXCHK(hipMemsetAsync(seqs + hb.seq_bytes, 0, kDevPad, s));
    FXCHK(hipMemcpyAsync(d.offs[slot].p, hb.offsets, (hb.n + 1) * 8, hipMemcpyHostToDevice, s));
    FXCHK(hipStreamSynchronize(s));
    uint64_t mx = 0;
    for (uint64_t i = 0; i < hb.n; ++i) mx = std::max(mx, hb.offsets[i + 1] - hb.offsets[i]);
    out->n = hb.n;
    out->seq_bytes = hb.seq_bytes;
    out->seqs = seqs;
    out->offsets = d.offs[slot].as<uint64_t>();
    out->host_offsets = hb.offsets;
    out->max_len = mx;
    out->ids = hb.ids;
    out->id_offsets = hb.id_offsets;
    out->descs = hb.descs;
    out->desc_offsets = hb.desc_offsets;
    out->parsed_on_device = 0;
    return XS_OK;
}

// The streams and events of a new device side.  The parse kernels are short
// and sit between the caller's probes of the previous batch: a high-priority
// stream lets their workgroups in as soon as the probe frees a slot, instead
// of after the whole probe.  The text DMA has a stream of its own, so the
// next window's copy never queues behind this window's parse.
hipError_t make_streams(StreamSet& ss) {
    int least = 0, greatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&ss.stream, hipStreamNonBlocking, greatest);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ss.copy, hipStreamNonBlocking);
    ss.each_event([&](hipEvent_t& ev) {
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    });
    return e;
}

}  // namespace
}  // namespace xs::fx

extern "C" {

int xs_fastx_open_device(const char* path, int format, int threads, int device, uint32_t part, uint32_t parts,
                         xs_fastx** out) {
    return xs::guard([&]() -> int {
        if (int rc = xs_fastx_open_range(path, format, threads, 0, part, parts, out)) return rc;
        xs_fastx* r = *out;
        r->release_dev = put_devside;
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess && !(r->dev = take_devside(device))) {
            r->dev = new DevSide();
            r->dev->ss.device = device;
            if (!take_streams(r->dev->ss)) e = make_streams(r->dev->ss);
        }
        if (e == hipSuccess) return XS_OK;
        xs_fastx_close(r);
        *out = nullptr;
        return xs::set_error(XS_ERR_HIP, hipGetErrorString(e));
    });
}

int xs_fastx_wait_host(const xs_fastx_dbatch* b) {
    return xs::guard([&]() -> int {
        if (!b) return xs::set_error(XS_ERR_ARG, "null argument");
        if (b->host_ready) FXCHK(hipEventSynchronize(static_cast<hipEvent_t>(b->host_ready)));
        return XS_OK;
    });
}

int xs_fastx_next_device(xs_fastx* r, uint64_t max_text_bytes, xs_fastx_dbatch* out) {
    return xs::guard([&]() -> int {
        if (!r || !out) return xs::set_error(XS_ERR_ARG, "null argument");
        if (!r->dev) return xs::set_error(XS_ERR_ARG, "reader was not opened with xs_fastx_open_device");
        memset(out, 0, sizeof(*out));
        DevSide& d = *r->dev;
        FXCHK(hipSetDevice(d.ss.device));
        if (fx_trace()) fprintf(stderr, "[fastx-device] t=%.2f next_device\n", fx_ms());
        const int slot = d.flip;
        d.flip ^= 1;
        if (r->format == XS_FASTX_FASTQ && r->wrapped) {  // records cannot be cut by pattern: host parser
            xs_fastx_batch hb;
            if (int rc = xs_fastx_next(r, max_text_bytes, &hb)) return rc;
            if (int rc = upload_host_batch(r, hb, slot, out)) return rc;
            out->text_offset = hb.text_offset;
            out->text_bytes = hb.text_bytes;
            return XS_OK;
        }
        const char* end = r->base + r->stop;
        for (;;) {
            if (r->cur >= r->stop) {
                drain_loads(d);
                out->text_offset = r->cur;
                out->text_bytes = r->stop;
                return XS_OK;
            }
            const char* lo = r->base + r->cur;
            const char* hi = window_end(r, lo, end, window_budget(max_text_bytes, r->windows));
            const size_t flo = (size_t)(lo - r->base), fhi = (size_t)(hi - r->base);
            const double t0 = fx_ms();
            bool prefetched = false;
            int ts = 0;
            if (int rc = text_for(r, flo, fhi, &ts, &prefetched)) return rc;
            const double t1 = fx_ms();
            r->cur = fhi;
            ++r->windows;
            // The next window's text loads into the other slot while this one is
            // parsed and the caller works on the batch; the one after it goes
            // into this window's slot once this parse is done.
            size_t n1_hi = 0;  // end of the next window
            if (r->cur < r->stop)
                n1_hi = (size_t)(window_end(r, r->base + r->cur, end, window_budget(max_text_bytes, r->windows)) - r->base);
            if (n1_hi && !is_queued(d, r->cur)) queue_window(r, r->cur, n1_hi);
            bool ok = false;
            g_fx = FxTimes{};
            if (int rc = parse_on_device(r, flo, fhi, slot, ts, &ok, out)) return rc;
            if (n1_hi && n1_hi < r->stop && !is_queued(d, n1_hi))  // this slot's text is free now
                queue_window(r, n1_hi,
                             (size_t)(window_end(r, r->base + n1_hi, end, window_budget(max_text_bytes, r->windows + 1)) -
                                      r->base));
            if (fx_trace())
                fprintf(stderr,
                        "[fastx-device] t=%.2f window %zu+%zu: text %s load %.2f ms, wait %.2f ms | count %.2f records %.2f "
                        "copy %.2f ms | %s\n",
                        t0, flo, fhi - flo, prefetched ? "prefetched" : "inline", d.load_ms[ts], t1 - t0, g_fx.count,
                        g_fx.records, g_fx.copy, ok ? "device" : "host parser");
            if (!ok) {  // the host parser's batch for exactly this window
                int nparts = 0;
                if (int rc = parse_window(r, lo, hi, &nparts)) return rc;
                Batch& bt = r->batch[r->flip];
                r->flip ^= 1;
                if (int rc = pack_parts(r, bt, nparts)) return rc;
                xs_fastx_batch hb;
                memset(&hb, 0, sizeof(hb));
                fill_host_batch(r, bt, &hb);
                if (int rc = upload_host_batch(r, hb, slot, out)) return rc;
            }
            if (out->n) {
                r->records += out->n;
                out->text_offset = r->cur;
                out->text_bytes = r->stop;
                if (fx_trace()) fprintf(stderr, "[fastx-device] t=%.2f return n=%llu\n", fx_ms(), (unsigned long long)out->n);
                return XS_OK;
            }
            memset(out, 0, sizeof(*out));  // no record in this window (text before the first one)
        }
    });
}

}  // extern "C"
