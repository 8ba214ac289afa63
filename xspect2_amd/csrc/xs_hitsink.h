// xs_hitsink.h — hit rows back to a host array, behind the probe, and the host's own passes over
// hit rows.  Included by xs_query.cpp only.
#pragma once
#include <sys/mman.h>

#include <condition_variable>
#include <deque>

#include "xs_host.h"

namespace xs {

// memcpy on up to `threads` host threads.
inline void par_memcpy(void* dst, const void* src, size_t n, int threads) {
    par_ranges(n, 4u << 20, threads, [=](int, uint64_t a, uint64_t e) {
        memcpy(static_cast<char*>(dst) + a, static_cast<const char*>(src) + a, e - a);
    });
}

// Ask for transparent huge pages over the page-aligned part of a pageable
// host destination the library is about to fill.  On the MI355X boxes the
// first write to fresh 4 KiB pages costs ~70 ms per 400 MB from one thread and
// ~34 ms from eight (the faults serialise); over 2 MiB pages it is ~25 ms from
// one thread and ~3.6 ms from eight (profiles/r05k_thp.json,
// tools/thp_probe.py), and the copy-out already writes from eight threads.
// Advisory only: pages already present stay as they are, and a mapping that
// cannot take the advice (file-backed, hugetlbfs) is left alone.
inline void advise_huge_pages(void* p, size_t bytes) {
    constexpr uintptr_t kPage = 4096;
    const uintptr_t a = (reinterpret_cast<uintptr_t>(p) + kPage - 1) & ~(kPage - 1);
    const uintptr_t e = (reinterpret_cast<uintptr_t>(p) + bytes) & ~(kPage - 1);
    if (e > a + (4u << 20)) (void)madvise(reinterpret_cast<void*>(a), e - a, MADV_HUGEPAGE);
}

// A host call's hit rows go to the caller's array on a worker thread while the
// bank stream probes the next chunks (the main thread only launches): each
// chunk's rows, in the wire width (uint8 / uint16 narrowed on the device when
// every read's sampled k-mers fit, else uint32), are cut into pieces of
// kSinkPiece bytes, DMA'd on d2h_stream into a ring of three pinned slots (two
// pieces in flight while a third is copied out) and copied by host threads
// into the caller's array, widened to its element width where the wire is
// narrower.  A pinned destination of the wire width takes the DMA directly.
// xs_query's uint32 matrix of 1 M reads x 100 docs thus crosses PCIe as 100 MB
// of uint8 instead of 400 MB, and its copy-out overlaps the probe.
constexpr size_t kSinkPiece = 32u << 20;
constexpr int kSinkSlots = 3;

template <class S, class D>
void widen_rows(D* dst, const S* src, size_t n, int threads) {
    par_ranges(n, 1u << 20, threads, [=](int, uint64_t a, uint64_t e) {
        for (uint64_t i = a; i < e; ++i) dst[i] = (D)src[i];
    });
}

// dst[i] = src[i] as hit_bytes-wide counts that the caller checked to fit, on this thread (a small call's rows)
inline void narrow_rows(void* dst, int hit_bytes, const uint32_t* src, size_t n) {
    if (hit_bytes == 4) memcpy(dst, src, n * 4);
    else if (hit_bytes == 2)
        for (size_t i = 0; i < n; ++i) static_cast<uint16_t*>(dst)[i] = (uint16_t)src[i];
    else
        for (size_t i = 0; i < n; ++i) static_cast<uint8_t*>(dst)[i] = (uint8_t)src[i];
}

// best_doc_kernel's rule on host rows (a small call's): per row of `cols` counts the document holding the
// unique maximum, else kBestAmbiguous; best_hits (may be null) takes the maximum.
inline void best_rows(const uint32_t* rows, uint64_t n, uint64_t cols, uint32_t* best_doc, uint32_t* best_hits) {
    for (uint64_t r = 0; r < n; ++r) {
        const uint32_t* row = rows + r * cols;
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
}

// Narrowest transport width (bytes) of hit counts up to max_count, at most `out`.
inline int wire_width(uint64_t max_count, int out) {
    const int w = max_count <= 0xFFu ? 1 : max_count <= 0xFFFFu ? 2 : 4;
    return std::min(w, out);
}

class HitSink {
  public:
    // rows of `cols` counts: on the device at `src` (wire bytes each), to `host` (out bytes each)
    HitSink(xs_bank* b, void* host, const void* src, uint64_t cols, int wire, int out)
        : b_(b), host_(static_cast<uint8_t*>(host)), src_(static_cast<const uint8_t*>(src)), cols_(cols),
          wire_(wire), out_(out) {}
    // an early return of the caller: the copies stop, and the caller's error stays the one reported
    ~HitSink() { join(); }

    int start(uint64_t total_bytes_out) {
        // small: one DMA into pageable memory is as fast as staging it
        if (wire_ == out_) direct_ = total_bytes_out < 2 * kSinkPiece || is_pinned_host(host_);
        if (!direct_) {  // a pageable destination, filled by the copy-out threads
            advise_huge_pages(host_, total_bytes_out);
            for (int s = 0; s < kSinkSlots; ++s) {
                if (int rc = b_->stage[s].ensure(kSinkPiece)) return rc;
                if (!b_->stage_ev[s]) HIPCHK(hipEventCreateWithFlags(&b_->stage_ev[s], hipEventDisableTiming));
            }
        }
        th_ = std::thread([this] { run(); });
        return XS_OK;
    }
    // rows [r0, r1) are complete on the device once `ev` has fired
    void push(uint64_t r0, uint64_t r1, hipEvent_t ev) {
        {
            std::lock_guard<std::mutex> g(mu_);
            q_.push_back(Job{r0, r1, ev});
        }
        cv_.notify_one();
    }
    // no more rows: wait for the copies; the worker's error, if any, becomes this thread's
    int finish() {
        join();
        return rc_ ? xs::set_error(rc_, err_.c_str()) : XS_OK;
    }

  private:
    void join() {
        if (!th_.joinable()) return;
        {
            std::lock_guard<std::mutex> g(mu_);
            closed_ = true;
        }
        cv_.notify_one();
        th_.join();
    }
    struct Job {
        uint64_t r0, r1;
        hipEvent_t ev;
    };
    struct Piece {
        int slot;
        uint64_t elem0, elems;  // first element and count
    };
    int copy_out(const Piece& p) {
        if (hipEventSynchronize(b_->stage_ev[p.slot]) != hipSuccess) return XS_ERR_HIP;
        const void* in = b_->stage[p.slot].p;
        const int t = host_threads();
        switch (wire_ * 8 + out_) {  // wire <= out, each 1, 2 or 4
            case 1 * 8 + 2: widen_rows(reinterpret_cast<uint16_t*>(host_) + p.elem0, static_cast<const uint8_t*>(in), p.elems, t); break;
            case 1 * 8 + 4: widen_rows(reinterpret_cast<uint32_t*>(host_) + p.elem0, static_cast<const uint8_t*>(in), p.elems, t); break;
            case 2 * 8 + 4: widen_rows(reinterpret_cast<uint32_t*>(host_) + p.elem0, static_cast<const uint16_t*>(in), p.elems, t); break;
            default: par_memcpy(host_ + p.elem0 * out_, in, p.elems * out_, t);  // wire == out
        }
        return XS_OK;
    }
    void fail_with(int rc, const char* what) {
        if (!rc_) {
            rc_ = rc;
            err_ = what;
        }
    }
    // the worker thread's body: a C++ exception in it (a failed allocation, a copy-out
    // task) becomes the call's error instead of ending the process
    void run() {
        try {
            copy_loop();
        } catch (const std::bad_alloc&) {
            fail_with(XS_ERR_NOMEM, "host memory allocation failed in the hit copier");
        } catch (const std::exception& e) {
            fail_with(XS_ERR_INTERNAL, e.what());
        } catch (...) {
            fail_with(XS_ERR_INTERNAL, "unknown C++ exception in the hit copier");
        }
        // whatever happened above: no DMA may still be writing a staging slot when the call returns
        if (hipStreamSynchronize(b_->d2h_stream) != hipSuccess) fail_with(XS_ERR_HIP, "hit D2H failed");
    }
    void copy_loop() {
        if (hipSetDevice(b_->device) != hipSuccess) return fail_with(XS_ERR_HIP, "hipSetDevice failed in the hit copier");
        std::deque<Piece> inflight;
        int next_slot = 0;
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [&] { return closed_ || !q_.empty(); });
                if (q_.empty()) break;
                j = q_.front();
                q_.pop_front();
            }
            if (rc_) continue;  // drain the queue after a failure
            hipError_t e = hipStreamWaitEvent(b_->d2h_stream, j.ev, 0);
            const uint64_t e0 = j.r0 * cols_, e1 = j.r1 * cols_;
            const uint64_t per = kSinkPiece / (uint64_t)wire_;
            for (uint64_t a = e0; e == hipSuccess && a < e1; a += per) {
                const uint64_t m = std::min(per, e1 - a);
                if (direct_) {
                    e = hipMemcpyAsync(host_ + a * out_, src_ + a * wire_, m * wire_, hipMemcpyDeviceToHost,
                                       b_->d2h_stream);
                    continue;
                }
                if ((int)inflight.size() == kSinkSlots - 1) {  // the oldest piece out of its slot first
                    if (int rc = copy_out(inflight.front())) {
                        fail_with(rc, "hit copy-out failed");
                        break;
                    }
                    inflight.pop_front();
                }
                const int slot = next_slot;
                next_slot = (next_slot + 1) % kSinkSlots;
                e = hipMemcpyAsync(b_->stage[slot].p, src_ + a * wire_, m * wire_, hipMemcpyDeviceToHost, b_->d2h_stream);
                if (e == hipSuccess) e = hipEventRecord(b_->stage_ev[slot], b_->d2h_stream);
                inflight.push_back(Piece{slot, a, m});
            }
            if (e != hipSuccess) fail_with(XS_ERR_HIP, hipGetErrorString(e));
        }
        while (!inflight.empty() && !rc_) {
            if (int rc = copy_out(inflight.front())) fail_with(rc, "hit copy-out failed");
            inflight.pop_front();
        }
    }

    xs_bank* b_;
    uint8_t* host_;
    const uint8_t* src_;
    uint64_t cols_;
    int wire_, out_;
    bool direct_ = false;
    std::thread th_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Job> q_;
    bool closed_ = false;
    int rc_ = XS_OK;
    std::string err_;
};

}  // namespace xs
