// xs_fastx.cpp — native FASTA/FASTQ reader that feeds the probe path
// (SURVEY.md §8 f1).  It replaces Bio.SeqIO.parse, which the reference reaches
// through get_record_iterator (src/xspect/file_io.py:47-79) for every
// predict() on a file (probabilistic_filter_model.py:316-330).
//
// Record semantics, restated from Biopython's SimpleFastaParser and
// FastqGeneralIterator (Bio is not installed offline; the pure-Python
// restatement oracle/fastx.py is the checker, tests/test_fastx.py):
//   * lines end at '\n'; every line is right-stripped of ASCII whitespace;
//   * FASTA: text before the first '>' line is skipped; title = header minus
//     '>', id = first whitespace-separated token of the title ("" if none);
//     sequence = the record's lines joined, with ' ' and '\r' removed;
//   * FASTQ: blank lines between records are skipped; a header must start
//     with '@'; sequence lines run to the first line starting with '+' (whose
//     caption, if any, must equal the title); no ' ' or '\t' in the sequence;
//     quality lines are read until they hold >= len(sequence) characters and
//     must then hold exactly len(sequence).
//
// A batch covers a window of the memory-mapped file cut at a record start.
// The window is split at record starts into one part per thread, the parts
// are parsed concurrently and copied into one packed batch (bytes + offsets,
// the layout xs_query takes).  Two batches are double-buffered so the caller
// can probe batch i while batch i+1 is parsed.  FASTQ with wrapped sequence
// or quality lines cannot be split safely; such files are parsed by one
// thread.
//
// Device mode (xs_fastx_open_device): the host only copies each window's text
// into pinned memory (parallel pread) and on to HBM, overlapped with the
// caller's work on the previous batch; the records are found on the GPU
// (xs_fastx_dev.hip).  A window the device rules do not cover is parsed by the
// host parser instead, so both modes yield the same batches.
//
// This file holds the entry points of the host mode, the FASTA writer and the
// reader's three settings; the parser is in xs_fastx_parse.cpp, the device
// mode in xs_fastx_devside.cpp, what they share in xs_fastx.h.
#include "xs_fastx.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>

using namespace xs::fx;

xs_fastx::~xs_fastx() {
    if (release_dev) release_dev(dev);
    if (base && size) munmap(const_cast<char*>(base), size);
    if (fd >= 0) close(fd);
}

namespace xs::fx {

// XSPECT2_AMD_FX_FIRST_MB sets the first window (MiB, read once; default 16:
// file -> totals of 1 M reads 16.8-16.9 ms against 17.0-17.5 at 32 MiB and
// 35-48 at 8 MiB, profiles/r04_e2e_first_window.txt).
size_t first_window() {
    static const size_t w = [] {
        const char* e = getenv("XSPECT2_AMD_FX_FIRST_MB");
        const long v = e ? atol(e) : 0;
        return v > 0 ? (size_t)v << 20 : (size_t)16 << 20;
    }();
    return w;
}

// XSPECT2_AMD_FX_RING: pinned ring pieces (read once; default 32 = 128 MiB;
// 0 = a pinned buffer the size of each window, per text slot)
size_t ring_pieces() {
    static const size_t r = [] {
        const char* e = getenv("XSPECT2_AMD_FX_RING");
        const long v = e ? atol(e) : 32;
        return (size_t)std::max<long>(0, std::min<long>(v, (long)kRingMax));
    }();
    return r;
}

// XSPECT2_AMD_FASTX_TRACE set: one line per device window on stderr with the
// time of each phase (diagnostics of the device mode).
bool fx_trace() {
    static const bool on = getenv("XSPECT2_AMD_FASTX_TRACE") != nullptr;
    return on;
}

}  // namespace xs::fx

extern "C" {

int xs_fastx_open(const char* path, int format, int threads, int flags, xs_fastx** out) {
    return xs::guard([&]() -> int {
        return xs_fastx_open_range(path, format, threads, flags, 0, 1, out);
    });
}

int xs_fastx_open_range(const char* path, int format, int threads, int flags, uint32_t part, uint32_t parts,
                        xs_fastx** out) {
    return xs::guard([&]() -> int {
        if (!path || !out) return xs::set_error(XS_ERR_ARG, "null argument");
        if (parts == 0 || part >= parts) return xs::set_error(XS_ERR_ARG, "part must be < parts");
        if (format != XS_FASTX_FASTA && format != XS_FASTX_FASTQ)
            return xs::set_error(XS_ERR_ARG, "format must be XS_FASTX_FASTA or XS_FASTX_FASTQ");
        *out = nullptr;
        std::unique_ptr<xs_fastx> r(new xs_fastx());  // closes and unmaps on every way out
        auto io_error = [&](const char* what) { return xs::set_error(XS_ERR_IO, (std::string(what) + path).c_str()); };
        r->format = format;
        if ((r->fd = open(path, O_RDONLY)) < 0) return io_error("cannot open ");
        struct stat st;
        if (fstat(r->fd, &st) != 0) return io_error("cannot stat ");
        r->size = (size_t)st.st_size;
        if (r->size) {
            void* m = mmap(nullptr, r->size, PROT_READ, MAP_PRIVATE, r->fd, 0);
            if (m == MAP_FAILED) return io_error("cannot map ");
            r->base = static_cast<const char*>(m);
            (void)madvise(m, r->size, MADV_SEQUENTIAL);
        }
        int t = threads > 0 ? threads : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
        r->threads = std::min(t, 64);
        if (format == XS_FASTX_FASTQ && r->size) r->wrapped = fastq_wrapped(r->base, r->base + r->size);
        // Part p of P: the records whose first byte lies in [cut(p), cut(p+1)), cut(i)
        // = the first record start at or after size*i/P (cut(0) = 0, cut(P) = size).
        // Every record belongs to exactly one part, in file order.
        r->stop = r->size;
        if (parts > 1 && r->size) {
            const char* lo = r->base;
            const char* end = r->base + r->size;
            auto cut = [&](uint64_t i) -> size_t {
                if (i == 0) return 0;
                if (i >= parts) return r->size;
                const char* pos = lo + (size_t)((unsigned __int128)r->size * i / parts);
                const char* c = format == XS_FASTX_FASTA ? fasta_boundary(lo, pos, end)
                                : r->wrapped             ? fastq_boundary_sequential(lo, pos, end)
                                                         : fastq_boundary(lo, pos, end);
                return (size_t)(c - lo);
            };
            r->cur = cut(part);
            r->stop = std::max(r->cur, cut((uint64_t)part + 1));
        }
        for (auto& b : r->batch) {
            const bool pinned = (flags & XS_FASTX_PINNED) != 0;
            b.seqs.pinned = b.offs.pinned = pinned;
        }
        r->parts.resize((size_t)r->threads);
        *out = r.release();
        return XS_OK;
    });
}

int xs_fastx_next(xs_fastx* r, uint64_t max_text_bytes, xs_fastx_batch* out) {
    return xs::guard([&]() -> int {
        if (!r || !out) return xs::set_error(XS_ERR_ARG, "null argument");
        memset(out, 0, sizeof(*out));
        Batch& bt = r->batch[r->flip];
        r->flip ^= 1;
        bt.n = bt.seq_bytes = 0;
        const char* end = r->base + r->stop;
        int nparts = 0;
        // a window can hold no record (text before the first one): go on until
        // records are found or the file ends
        for (;;) {
            const char* lo = r->base + r->cur;
            const size_t budget = window_budget(max_text_bytes, r->windows);
            nparts = 0;
            if (lo < end) {
                ++r->windows;
                if (r->format == XS_FASTX_FASTQ && r->wrapped) {
                    // sequential: the parser itself stops at the first record past the budget
                    Part& pt = r->parts[0];
                    pt.clear();
                    parse_fastq(lo, end, budget, pt);
                    nparts = 1;
                    if (!pt.err.empty()) return xs::set_error(XS_ERR_FORMAT, pt.err.c_str());
                } else if (int rc = parse_window(r, lo, window_end(r, lo, end, budget), &nparts)) {
                    return rc;
                }
            }
            if (nparts) r->cur = (size_t)(r->parts[nparts - 1].stop - r->base);
            size_t got = 0;
            for (int i = 0; i < nparts; ++i) got += r->parts[i].lens.size();
            if (got || r->cur >= r->stop || !nparts) break;
        }
        if (int rc = pack_parts(r, bt, nparts)) return rc;
        r->records += bt.n;
        fill_host_batch(r, bt, out);
        return XS_OK;
    });
}

void xs_fastx_close(xs_fastx* r) { delete r; }

int xs_write_fasta(const char* path, int append, const char* seqs, const uint64_t* offsets, const char* descs,
                   const uint64_t* desc_offsets, const uint32_t* index, uint64_t n, uint32_t width) {
    return xs::guard([&]() -> int {
        if (!path || (n && (!seqs || !offsets || !desc_offsets))) return xs::set_error(XS_ERR_ARG, "null argument");
        if (width == 0) return xs::set_error(XS_ERR_ARG, "width must be >= 1");
        FILE* f = fopen(path, append ? "ab" : "wb");
        if (!f) return xs::set_error(XS_ERR_IO, (std::string("cannot open ") + path).c_str());
        const int T = (int)std::min<uint64_t>(16, std::max<uint64_t>(1, n / 4096));
        const uint64_t block = 1 << 15;
        std::vector<std::string> out((size_t)T);
        bool ok = true;
        for (uint64_t b0 = 0; b0 < n && ok; b0 += block) {
            const uint64_t b1 = std::min(n, b0 + block), per = (b1 - b0 + T - 1) / T;
            auto work = [&](int t) {
                std::string& o = out[t];
                o.clear();
                const uint64_t lo = b0 + per * t, hi = std::min(b1, lo + per);
                for (uint64_t i = lo; i < hi; ++i) {
                    const uint64_t r = index ? index[i] : i;
                    o += '>';
                    o.append(descs + desc_offsets[r], (size_t)(desc_offsets[r + 1] - desc_offsets[r]));
                    o += '\n';
                    const char* s = seqs + offsets[r];
                    const uint64_t len = offsets[r + 1] - offsets[r];
                    for (uint64_t p = 0; p < len; p += width) {
                        o.append(s + p, (size_t)std::min<uint64_t>(width, len - p));
                        o += '\n';
                    }
                }
            };
            xs::parallel_for(T, work);
            for (int t = 0; t < T && ok; ++t) ok = fwrite(out[t].data(), 1, out[t].size(), f) == out[t].size();
        }
        if (fclose(f) != 0) ok = false;
        if (!ok) return xs::set_error(XS_ERR_IO, (std::string("write failed: ") + path).c_str());
        return XS_OK;
    });
}

}  // extern "C"
