// xs_fastx.h — what the files of the FASTA/FASTQ reader share: the handle,
// its batches and the parser's functions (xs_fastx_parse.cpp), the entry
// points and settings (xs_fastx.cpp), and the device mode
// (xs_fastx_devside.cpp).  Host only; no kernel file includes it.
#pragma once
#include "../../include/xspect_hip.h"

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "xs_internal.h"

namespace xs::fx {

struct HostBuf {
    char* p = nullptr;
    size_t cap = 0;
    bool pinned = false;
    int ensure(size_t bytes) {  // contents are not preserved
        if (bytes <= cap && p) return XS_OK;
        release();
        const size_t want = std::max<size_t>(bytes + bytes / 4, 4096);
        if (!pinned) p = static_cast<char*>(malloc(want));
        else if (xs::pinned_alloc(want, reinterpret_cast<void**>(&p)) != XS_OK) p = nullptr;
        if (!p)
            return pinned ? xs::set_error(XS_ERR_HIP, "pinned allocation failed for the reader's batch buffer")
                          : xs::set_error(XS_ERR_ARG, "out of host memory for the reader's batch buffer");
        cap = want;
        return XS_OK;
    }
    void release() {
        if (p) {
            if (pinned) xs::pinned_free(p);
            else free(p);
        }
        p = nullptr;
        cap = 0;
    }
    ~HostBuf() { release(); }
};

// One thread's records.
struct Part {
    std::string seq, ids, descs;
    std::vector<uint64_t> lens, id_lens, desc_lens;
    std::string err;
    const char* stop = nullptr;  // where parsing ended (next record start)
    void clear() {  // capacities are kept
        for (std::string* s : {&seq, &ids, &descs, &err}) s->clear();
        for (std::vector<uint64_t>* v : {&lens, &id_lens, &desc_lens}) v->clear();
        stop = nullptr;
    }
};

struct Batch {
    HostBuf seqs, offs, ids, id_offs, descs, desc_offs;
    uint64_t n = 0, seq_bytes = 0;
};

struct DevSide;  // the device mode's state (xs_fastx_devside.cpp)

}  // namespace xs::fx

struct xs_fastx {
    int format = XS_FASTX_FASTA;
    int threads = 1;
    bool wrapped = false;
    int fd = -1;
    const char* base = nullptr;
    size_t size = 0;   // mapped bytes
    size_t stop = 0;   // end of this reader's text (the file, or its part)
    size_t cur = 0;
    uint64_t records = 0;
    uint64_t windows = 0;  // windows consumed (window_budget's ramp)
    xs::fx::Batch batch[2];
    int flip = 0;
    std::vector<xs::fx::Part> parts;
    xs::fx::DevSide* dev = nullptr;                   // set by xs_fastx_open_device,
    void (*release_dev)(xs::fx::DevSide*) = nullptr;  // with the function that takes it back
    ~xs_fastx();
};

namespace xs::fx {

// ---- parser (xs_fastx_parse.cpp) -------------------------------------------
// FASTQ records of [p, end).  `budget`: stop at the first record that starts
// at or beyond p + budget once one record is held (0: no limit).
void parse_fastq(const char* p, const char* end, size_t budget, Part& out);
// Record start at or after `pos` in [lo, end): a FASTA '>' line, a four-line
// FASTQ record, or (wrapped FASTQ) the record walk from lo.
const char* fasta_boundary(const char* lo, const char* pos, const char* end);
const char* fastq_boundary(const char* lo, const char* pos, const char* end);
const char* fastq_boundary_sequential(const char* lo, const char* pos, const char* end);
bool fastq_wrapped(const char* p, const char* end);
size_t window_budget(uint64_t max_text_bytes, uint64_t k);
const char* window_end(const xs_fastx* r, const char* lo, const char* end, size_t budget);
int parse_window(xs_fastx* r, const char* lo, const char* hi, int* nparts);
int pack_parts(xs_fastx* r, Batch& bt, int nparts);
void fill_host_batch(const xs_fastx* r, const Batch& bt, xs_fastx_batch* out);

// ---- settings, each read once per process (xs_fastx.cpp) -------------------
constexpr size_t kRingMax = 64;  // most pinned ring pieces (DevSide::ring)
size_t first_window();           // bytes of a reader's first window
size_t ring_pieces();            // pinned ring pieces of the device mode, <= kRingMax
bool fx_trace();                 // [fastx-device] lines on stderr

}  // namespace xs::fx
