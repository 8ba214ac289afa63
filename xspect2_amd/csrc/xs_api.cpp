// xs_api.cpp — the C ABI (include/xspect_hip.h) beside bank files (xs_bank_io.cpp), queries (xs_query.cpp) and
// MLST (xs_mlst.cpp): errors, pinned host memory, device copies, handle information, profiling and options,
// handle teardown.
#include <sys/mman.h>

#include <cstdarg>
#include <cstdio>
#include <unordered_map>

#include "xs_host.h"

using namespace xs;

namespace {
thread_local std::string g_err;
std::mutex g_pin_mu;
std::unordered_map<void*, size_t> g_pins;  // registered mappings: start -> length
}  // namespace

int xs::fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int xs::set_error(int code, const char* msg) {
    g_err = msg;
    return code;
}

int xs::pinned_alloc(size_t bytes, void** out) {
    *out = nullptr;
    constexpr size_t kHuge = size_t(2) << 20;
    const size_t n = (std::max<size_t>(bytes, 1) + kHuge - 1) & ~(kHuge - 1);
    if (bytes >= kHuge) {
        const size_t len = n + kHuge;  // room to align the start to a 2 MiB page
        void* raw = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (raw != MAP_FAILED) {
            char* r = static_cast<char*>(raw);
            char* p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(r) + kHuge - 1) & ~(uintptr_t)(kHuge - 1));
            if (p > r) (void)munmap(r, (size_t)(p - r));           // the unaligned head
            if (r + len > p + n) (void)munmap(p + n, (size_t)(r + len - (p + n)));  // and tail
            (void)madvise(p, n, MADV_HUGEPAGE);
            // fault every page now, from several threads (2 MiB pages fault in parallel; the
            // registration below would otherwise fault them one by one)
            const int threads = (int)std::min<size_t>(8, std::max<size_t>(1, n / (size_t(16) << 20)));
            const size_t per = (n / kHuge + threads - 1) / threads * kHuge;
            xs::parallel_for(threads, [=](int t) {
                if (per * t < n) memset(p + per * t, 0, std::min(per, n - per * t));
            });
            if (hipHostRegister(p, n, hipHostRegisterDefault) == hipSuccess) {
                std::lock_guard<std::mutex> g(g_pin_mu);
                g_pins[p] = n;
                *out = p;
                return XS_OK;
            }
            (void)hipGetLastError();
            (void)munmap(p, n);
        }
    }
    const hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) {
        *out = nullptr;
        return fail(XS_ERR_HIP, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
    return XS_OK;
}

void xs::pinned_free(void* p) {
    if (!p) return;
    size_t n = 0;
    {
        std::lock_guard<std::mutex> g(g_pin_mu);
        auto it = g_pins.find(p);
        if (it != g_pins.end()) {
            n = it->second;
            g_pins.erase(it);
        }
    }
    if (n) {
        (void)hipHostUnregister(p);
        (void)munmap(p, n);
    } else {
        (void)hipHostFree(p);
    }
}

xs_bank::~xs_bank() {
    (void)hipSetDevice(device);
    if (ws_ev) (void)hipEventDestroy(ws_ev);
    for (hipStream_t st : {stream, copy_stream, d2h_stream})  // a failed open may have created none
        if (st) (void)hipStreamSynchronize(st);
    for (auto& ev : stage_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : hstage_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (bloom_ev) (void)hipEventDestroy(bloom_ev);
    for (auto& ev : chunk_ev) (void)hipEventDestroy(ev);
    for (auto& ev : events) {
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    for (auto& ev : pass_ev) (void)hipEventDestroy(ev);
    for (hipStream_t st : {stream, copy_stream, d2h_stream})
        if (st) (void)hipStreamDestroy(st);
}  // the DevBuf and PinnedBuf members free their memory

extern "C" {

int xs_version(void) { return 100; }

const char* xs_last_error(void) { return g_err.c_str(); }

int xs_device_count(int* count) {
    return xs::guard([&]() -> int {
        if (!count) return fail(XS_ERR_ARG, "null count");
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess) {
            *count = 0;
            return fail(XS_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
        }
        *count = n;
        return XS_OK;
    });
}

int xs_bank_set_term_size(xs_bank* b, uint32_t term_size) {
    return xs::guard([&]() -> int {
        if (!b) return fail(XS_ERR_ARG, "null argument");
        if (b->kind != XS_BANK_RBLOOM)
            return fail(XS_ERR_ARG, "COBS banks carry their term size in the file header");
        if (term_size < 1 || term_size > kMaxK)
            return fail(XS_ERR_UNSUPPORTED, "term_size %u unsupported on the device (1..%u)", term_size, kMaxK);
        std::lock_guard<std::mutex> lk(b->mu);
        b->k = term_size;
        return XS_OK;
    });
}

int xs_bank_info(const xs_bank* b, xs_bank_info_t* o) {
    return xs::guard([&]() -> int {
        if (!b || !o) return fail(XS_ERR_ARG, "null argument");
        memset(o, 0, sizeof(*o));
        o->kind = b->kind;
        o->device = b->device;
        o->term_size = b->k;
        o->num_hashes = b->h;
        o->canonicalize = b->canonicalize;
        o->num_docs = b->D;
        o->num_groups = b->kind == XS_BANK_RBLOOM ? 0 : b->G;
        o->page_size = b->page;
        o->signature_rows = b->sig_total();
        o->bloom_bits = b->kind == XS_BANK_RBLOOM ? b->nbytes * 8 : 0;
        o->device_bytes = b->dev_bytes;
        o->device_row_pitch = b->pitch;
        return XS_OK;
    });
}

int xs_bank_signature_sizes(const xs_bank* b, uint64_t* out, uint64_t n) {
    return xs::guard([&]() -> int {
        if (!b || !out) return fail(XS_ERR_ARG, "null argument");
        if (b->kind == XS_BANK_RBLOOM) return fail(XS_ERR_ARG, "rbloom banks have no signature groups");
        if (n != b->sig.size()) return fail(XS_ERR_ARG, "bank has %zu groups, %llu requested", b->sig.size(),
                                            (unsigned long long)n);
        for (uint64_t g = 0; g < n; ++g) out[g] = b->sig[g];
        return XS_OK;
    });
}

const char* xs_bank_doc_name(const xs_bank* b, uint64_t i) {
    return xs::guard([&]() -> const char* {
        if (!b || i >= b->names.size()) {
            fail(XS_ERR_ARG, "doc index out of range");
            return nullptr;
        }
        return b->names[i].c_str();
    });
}

int xs_memcpy_to_host(void* host, const void* dev, uint64_t bytes) {
    return xs::guard([&]() -> int {
        if (bytes && (!host || !dev)) return fail(XS_ERR_ARG, "null argument");
        if (bytes) HIPCHK(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
        return XS_OK;
    });
}

int xs_memcpy_device(void* dst, const void* src, uint64_t bytes, void* stream) {
    return xs::guard([&]() -> int {
        if (bytes && (!dst || !src)) return fail(XS_ERR_ARG, "null argument");
        if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
        return XS_OK;
    });
}

int xs_host_alloc(uint64_t bytes, void** out) {
    return xs::guard([&]() -> int {
        if (!out) return fail(XS_ERR_ARG, "null argument");
        return xs::pinned_alloc(bytes, out);
    });
}

void xs_host_free(void* p) {
    xs::guard([&] { xs::pinned_free(p); });
}

int xs_gather_reads_device(const void* d_seqs, const uint64_t* d_offsets, const uint32_t* d_index, uint64_t m,
                           void* d_out_seqs, const uint64_t* d_out_offsets, void* stream) {
    return xs::guard([&]() -> int {
        if (m && (!d_seqs || !d_offsets || !d_index || !d_out_seqs || !d_out_offsets))
            return fail(XS_ERR_ARG, "null argument");
        HIPCHK(launch_gather_reads(static_cast<const uint8_t*>(d_seqs), d_offsets, d_index, m,
                                   static_cast<uint8_t*>(d_out_seqs), d_out_offsets, static_cast<hipStream_t>(stream)));
        return XS_OK;
    });
}

int xs_best_device(const uint32_t* d_hits, uint64_t n, uint64_t num_docs, uint32_t* d_best_doc,
                   uint32_t* d_best_hits, void* stream) {
    return xs::guard([&]() -> int {
        if ((!d_hits || !d_best_doc) && n) return fail(XS_ERR_ARG, "null argument");
        if (num_docs == 0) return fail(XS_ERR_ARG, "num_docs must be >= 1");
        HIPCHK(launch_best_doc(d_hits, n, num_docs, d_best_doc, d_best_hits, static_cast<hipStream_t>(stream)));
        return XS_OK;
    });
}

int xs_bank_set_profiling(xs_bank* b, int on) {
    return xs::guard([&]() -> int {
        if (!b) return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(b->mu);
        if (on && !b->profiling) {
            HIPCHK(hipSetDevice(b->device));
            if (int rc = b->rows_read.ensure(sizeof(uint64_t))) return rc;
            HIPCHK(hipMemsetAsync(b->rows_read.p, 0, sizeof(uint64_t), b->stream));
            HIPCHK(hipStreamSynchronize(b->stream));
        }
        if (on != 0 && !b->profiling) {  // a fresh profiling session: no marks left from an earlier one
            b->pass_used = 0;
            b->events_used = 0;
        }
        b->profiling = on != 0;
        return XS_OK;
    });
}

int xs_bank_probe_rows(xs_bank* b, uint64_t* rows) {
    return xs::guard([&]() -> int {
        if (!b || !rows) return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(b->mu);
        *rows = 0;
        if (b->kind != XS_BANK_RBLOOM || !b->rows_read.p) return XS_OK;
        HIPCHK(hipSetDevice(b->device));
        HIPCHK(hipDeviceSynchronize());  // probes may have run on a caller's stream
        HIPCHK(hipMemcpy(rows, b->rows_read.p, sizeof(uint64_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemset(b->rows_read.p, 0, sizeof(uint64_t)));
        return XS_OK;
    });
}

int xs_bank_probe_path(const xs_bank* b, int* path) {
    return xs::guard([&]() -> int {
        if (!b || !path) return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(const_cast<xs_bank*>(b)->mu);  // after any query in flight on the handle
        *path = b->last_path;
        return XS_OK;
    });
}

// Copies a NUL-terminated name (list) into the caller's buffer.
static int copy_names(const char* src, size_t len, char* buf, size_t cap) {
    if (len + 1 > cap) return fail(XS_ERR_ARG, "buffer too small");
    memcpy(buf, src, len);
    buf[len] = '\0';
    return XS_OK;
}

int xs_bank_probe_kernel(const xs_bank* b, char* buf, size_t cap) {
    return xs::guard([&]() -> int {
        if (!b || !buf) return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(const_cast<xs_bank*>(b)->mu);  // after any query in flight on the handle
        return copy_names(b->last_kernel, strlen(b->last_kernel), buf, cap);
    });
}

int xs_probe_kernel_names(char* buf, size_t cap) {
    return xs::guard([&]() -> int {
        if (!buf) return fail(XS_ERR_ARG, "null argument");
        std::string names;
        probe_kernel_names(names);
        return copy_names(names.data(), names.size(), buf, cap);
    });
}

int xs_bank_set_probe_options(xs_bank* b, const xs_probe_options_t* o) {
    return xs::guard([&]() -> int {
        if (!b || !o) return fail(XS_ERR_ARG, "null argument");
        if (o->cobs_part < 0 || o->cobs_part > 4) return fail(XS_ERR_ARG, "cobs_part must be 0..4");
        if (o->bloom_part < 0 || o->bloom_part > 3) return fail(XS_ERR_ARG, "bloom_part must be 0..3");
        if (o->workspace_mib < 1) return fail(XS_ERR_ARG, "workspace_mib must be >= 1");
        if (o->small_calls != 0 && o->small_calls != 1) return fail(XS_ERR_ARG, "small_calls must be 0 or 1");
        std::lock_guard<std::mutex> lk(b->mu);  // after any query in flight on the handle
        b->opt.cobs_part = o->cobs_part;
        b->opt.bloom_part = o->bloom_part;
        b->opt.workspace_mib = o->workspace_mib;
        b->opt.small_calls = o->small_calls;
        return XS_OK;
    });
}

int xs_bank_workspace_bytes(const xs_bank* b, uint64_t* held, uint64_t* peak) {
    return xs::guard([&]() -> int {
        if (!b || !held || !peak) return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(const_cast<xs_bank*>(b)->mu);
        *held = b->ws_acct.held;
        *peak = b->ws_acct.peak;
        return XS_OK;
    });
}

int xs_bank_get_probe_options(const xs_bank* b, xs_probe_options_t* o) {
    return xs::guard([&]() -> int {
        if (!b || !o) return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(const_cast<xs_bank*>(b)->mu);
        o->cobs_part = b->opt.cobs_part;
        o->bloom_part = b->opt.bloom_part;
        o->workspace_mib = b->opt.workspace_mib;
        o->small_calls = b->opt.small_calls;
        return XS_OK;
    });
}

int xs_bank_last_probe_ms(xs_bank* b, float* ms) {
    return xs::guard([&]() -> int {
        if (!b || !ms) return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(b->mu);
        if (b->events_used == 0) return fail(XS_ERR_ARG, "no profiled query on this handle");
        HIPCHK(hipSetDevice(b->device));
        auto& ev = b->events[b->events_used - 1];
        HIPCHK(hipEventSynchronize(ev.second));
        HIPCHK(hipEventElapsedTime(ms, ev.first, ev.second));
        return XS_OK;
    });
}

int xs_bank_probe_stats(xs_bank* b, uint64_t* count, double* total_ms, float* max_ms) {
    return xs::guard([&]() -> int {
        if (!b || !count || !total_ms) return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(b->mu);
        HIPCHK(hipSetDevice(b->device));
        double tot = 0.0;
        float mx = 0.0f;
        for (size_t i = 0; i < b->events_used; ++i) {
            float ms = 0.0f;
            HIPCHK(hipEventSynchronize(b->events[i].second));
            HIPCHK(hipEventElapsedTime(&ms, b->events[i].first, b->events[i].second));
            tot += ms;
            mx = ms > mx ? ms : mx;
        }
        *count = b->events_used;
        *total_ms = tot;
        if (max_ms) *max_ms = mx;
        b->events_used = 0;
        return XS_OK;
    });
}

int xs_bank_pass_stats(xs_bank* b, double* ms, uint64_t* count) {
    return xs::guard([&]() -> int {
        if (!b || !ms || !count) return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(b->mu);
        HIPCHK(hipSetDevice(b->device));
        for (int t = 0; t < kPassTags; ++t) {
            ms[t] = 0.0;
            count[t] = 0;
        }
        for (size_t i = 1; i < b->pass_used; ++i) {
            const int t = b->pass_tag[i];
            if (t < 0 || t >= kPassTags) continue;  // a query's opening mark
            float x = 0.0f;
            HIPCHK(hipEventSynchronize(b->pass_ev[i]));
            HIPCHK(hipEventElapsedTime(&x, b->pass_ev[i - 1], b->pass_ev[i]));
            ms[t] += x;
            ++count[t];
        }
        b->pass_used = 0;
        return XS_OK;
    });
}

void xs_bank_close(xs_bank* b) {
    xs::guard([&] {
        if (!b) return;
        (void)hipSetDevice(b->device);
        if (b->ws_used) (void)hipEventSynchronize(b->ws_ev);  // the last call's stream may be the caller's
        delete b;
    });
}

}  // extern "C"
