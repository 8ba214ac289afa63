// xs_bank_io.cpp — bank files and device residency: the COBS / rbloom file formats, the device image, payloads
// streamed between files and the device through a ring of pinned slots, the open / create / save entry points.
// Headers are read, and every geometry checked, by xs_bank_header.cpp (host only, no HIP): what it refuses is
// refused before a handle exists and before the first HIP call here.
//
// Bank file layouts (restated; COBS and rbloom are not available offline, see
// DESIGN.md "Oracle" — parity with their real files is unpinned):
//   COBS classic  "COBS:CLASSIC_INDEX" u32 version=1, u32 num_docs, u32 term_size,
//                 u8 canonicalize, u64 signature_size, u64 num_hashes,
//                 num_docs x (name '\n'), "CLASSIC_INDEX",
//                 then signature_size rows of ceil(num_docs/8) bytes
//                 (doc d = byte d>>3, bit d&7).
//   COBS compact  "COBS:COMPACT_INDEX" u32 version=1, u32 term_size, u8 canonicalize,
//                 u64 num_groups, num_groups x (u64 signature_size, u64 num_hashes),
//                 u64 page_size, u32 num_docs, names, "COMPACT_INDEX", zero pad to a
//                 multiple of page_size; then per group signature_size rows of
//                 page_size bytes (group g = docs [8*page_size*g, 8*page_size*(g+1))).
//   rbloom        u64 little-endian K, then the filter bytes (bit i = byte i>>3,
//                 bit i&7).
// On the device every row is padded to a 16, 32 or 64-byte pitch, or to a
// multiple of 128 bytes: one row of a group is whole aligned dwordx4 chunks
// (128 docs each) and never straddles a 128-byte line.
#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <fstream>
#include <memory>

#include "xs_bank_header.h"
#include "xs_host.h"

using namespace xs;

namespace {

const char kClassicMagic[] = "CLASSIC_INDEX";
const char kCompactMagic[] = "COMPACT_INDEX";

// The device's limits as the header unit restates them.
static_assert(kHeaderMaxK == kMaxK && kHeaderMaxHashes == kMaxHashes, "xs_bank_header.h and xs_internal.h disagree");

// a refusal of the header unit as the calling thread's error; `path` names the file, if any
int refused(int rc, const char* path, const std::string& err) {
    return path ? fail(rc, "%s: %s", path, err.c_str()) : fail(rc, "%s", err.c_str());
}

// The LDS counters of a probe block hold every doc of the bank (after the header unit's checks).
int check_lds_budget(uint64_t D, const char* path) {
    int wpb;
    size_t lds;
    if (D > UINT32_MAX || probe_blocks(D, &wpb, &lds) != 0)
        return refused(XS_ERR_UNSUPPORTED, path,
                       std::to_string((unsigned long long)D) + " documents exceed the LDS counter budget");
    return XS_OK;
}

// The header of `path`, read and checked on the host alone (xs_bank_header.h): the file's layout, not yet
// whether one handle can hold all its docs (check_lds_budget, which xs_bank_open applies to the whole bank and
// xs_bank_open_docs to its slice only).
int read_checked_header(const char* path, int kind, BankGeometry* g) {
    std::string err;
    if (int rc = read_bank_header(path, kind, g, &err)) return refused(rc, path, err);
    return XS_OK;
}

// A handle of a checked geometry (its names moved out of g); no device work yet.
std::unique_ptr<xs_bank> bank_of(int device, BankGeometry& g) {
    auto b = std::make_unique<xs_bank>(device, g.kind);
    b->k = g.k;
    b->h = (uint32_t)g.h;  // 1..kMaxHashes
    b->canonicalize = g.canonicalize;
    b->D = g.D;
    b->G = g.G;
    b->page = g.page;
    b->sig = g.sig;
    b->names = std::move(g.names);
    b->nbytes = g.nbytes;
    b->pitch = g.pitch;
    b->dev_bytes = g.dev_bytes;
    return b;
}

// Allocate the (zeroed) device image (b->dev_bytes, from the checked geometry) and group table.
int alloc_image(xs_bank* b) {
    HIPCHK(hipSetDevice(b->device));
    if (!b->stream) HIPCHK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    if (int rc = b->image.ensure(b->dev_bytes)) return rc;
    HIPCHK(hipMemsetAsync(b->image.p, 0, b->dev_bytes, b->stream));
    if (b->kind != XS_BANK_RBLOOM) {
        std::vector<GroupDesc> gd(b->G);
        uint64_t base = 0;
        for (uint64_t g = 0; g < b->G; ++g) {
            gd[g].sig = b->sig[g];
            gd[g].magic = barrett_magic(b->sig[g]);
            gd[g].base = base;
            base += b->sig[g] * b->pitch;
        }
        if (int rc = b->groups.ensure(sizeof(GroupDesc) * b->G)) return rc;
        HIPCHK(hipMemcpyAsync(b->groups.p, gd.data(), sizeof(GroupDesc) * b->G,
                              hipMemcpyHostToDevice, b->stream));
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    return XS_OK;
}

// FILE layout payload (host) -> device image.
int upload_payload(xs_bank* b, const void* host, uint64_t nbytes) {
    if (nbytes != b->payload_bytes())
        return fail(XS_ERR_ARG, "payload of %llu bytes, bank expects %llu",
                    (unsigned long long)nbytes, (unsigned long long)b->payload_bytes());
    HIPCHK(hipSetDevice(b->device));
    if (int rc = ws_enter(b, b->stream)) return rc;
    if (b->kind == XS_BANK_RBLOOM || b->pitch == b->page) {
        HIPCHK(hipMemcpyAsync(b->image.p, host, nbytes, hipMemcpyHostToDevice, b->stream));
    } else {
        if (int rc = b->tmp.ensure(nbytes)) return rc;
        HIPCHK(hipMemcpyAsync(b->tmp.p, host, nbytes, hipMemcpyHostToDevice, b->stream));
        HIPCHK(launch_repack(b->tmp.as<uint8_t>(), b->page, b->image.as<uint8_t>(), b->pitch,
                             b->sig_total(), b->page, b->stream));
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    return XS_OK;
}

int download_payload(xs_bank* b, void* host, uint64_t nbytes) {
    if (nbytes != b->payload_bytes())
        return fail(XS_ERR_ARG, "buffer of %llu bytes, payload is %llu",
                    (unsigned long long)nbytes, (unsigned long long)b->payload_bytes());
    HIPCHK(hipSetDevice(b->device));
    if (int rc = ws_enter(b, b->stream)) return rc;
    if (b->kind == XS_BANK_RBLOOM || b->pitch == b->page) {
        HIPCHK(hipMemcpyAsync(host, b->image.p, nbytes, hipMemcpyDeviceToHost, b->stream));
    } else {
        if (int rc = b->tmp.ensure(nbytes)) return rc;
        HIPCHK(launch_repack(b->image.as<uint8_t>(), b->pitch, b->tmp.as<uint8_t>(), b->page,
                             b->sig_total(), b->page, b->stream));
        HIPCHK(hipMemcpyAsync(host, b->tmp.p, nbytes, hipMemcpyDeviceToHost, b->stream));
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    return XS_OK;
}

// ---- bank payloads straight from their files ------------------------------
// A model load (ProbabilisticFilterModel.load, probabilistic_filter_model.py:
// 351-391: cobs.Search(path) reads the whole index) moved the payload through
// a zero-filled std::vector, one ifstream read and a pageable H2D copy: 169 ms
// for config 2's 0.5 GB file (2.9 GB/s, profiles/r05q_open.json).  Here the
// file is read in pieces by up to 8 threads (pread) into a ring of pinned
// slots, each piece sent by DMA while the next is read.
constexpr uint64_t kLoadPiece = 32u << 20;
constexpr int kLoadSlots = 3;

// The ring: kLoadSlots pinned slots with an event each, for DMA on stream s.  On every
// exit path no DMA may still touch a slot when the ring is freed: s is drained first.
struct PinnedRing {
    hipStream_t s;
    PinnedBuf slot[kLoadSlots];
    hipEvent_t ev[kLoadSlots] = {};
    int init(uint64_t piece) {
        for (int i = 0; i < kLoadSlots; ++i) {
            if (int rc = slot[i].ensure(piece)) return rc;
            HIPCHK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        }
        return XS_OK;
    }
    uint8_t* at(int i) const { return static_cast<uint8_t*>(slot[i].p); }
    ~PinnedRing() {
        (void)hipStreamSynchronize(s);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

struct FdCloser {  // closes on every exit path unless fd was set to -1
    int fd;
    ~FdCloser() {
        if (fd >= 0) ::close(fd);
    }
};

// run(a, e, &ok) over the ranges of [0, n) of up to `threads` (<= 8) threads, at least
// 4 MiB each; false if any range failed
template <class F>
bool par_io(uint64_t n, int threads, F run) {
    const int T = (int)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)threads, 8, n / (4u << 20)}));
    const uint64_t per = (n + T - 1) / T;
    bool ok[8] = {true, true, true, true, true, true, true, true};
    xs::parallel_for(T, [&](int t) {
        const uint64_t a = per * (uint64_t)t;
        if (a < n) run(a, std::min(n, a + per), &ok[t]);
    });
    for (bool o : ok)
        if (!o) return false;
    return true;
}

// [off, off + n) of fd into dst, split over up to `threads` threads; false on a
// read error or a short file
bool pread_all(int fd, uint8_t* dst, uint64_t n, uint64_t off, int threads) {
    auto run = [=](uint64_t a, uint64_t e, bool* ok) {
        while (a < e) {
            const ssize_t got = pread(fd, dst + a, (size_t)(e - a), (off_t)(off + a));
            if (got <= 0) {
                if (got < 0 && errno == EINTR) continue;
                *ok = false;
                return;
            }
            a += (uint64_t)got;
        }
        *ok = true;
    };
    return par_io(n, threads, run);
}

// nbytes of `path` from byte `pos`, in pieces of `piece` bytes (the last one shorter) read by
// up to 8 threads into a ring of pinned slots; emit(off, m, slot) enqueues piece [off, off + m)'s
// transfer out of its slot on b->stream, which is synchronised on return
template <class Emit>
int stream_file(xs_bank* b, const char* path, uint64_t pos, uint64_t nbytes, uint64_t piece, Emit emit) {
    const int fd = ::open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return fail(XS_ERR_IO, "cannot open %s", path);
    FdCloser closer{fd};
    PinnedRing ring{b->stream};
    piece = std::min<uint64_t>(piece, std::max<uint64_t>(nbytes, 1));
    if (int rc = ring.init(piece)) return rc;
    uint64_t i = 0;
    for (uint64_t off = 0; off < nbytes; off += piece, ++i) {
        const int s = (int)(i % kLoadSlots);
        if (i >= (uint64_t)kLoadSlots) HIPCHK(hipEventSynchronize(ring.ev[s]));  // the slot's last DMA is done
        const uint64_t m = std::min(piece, nbytes - off);
        if (!pread_all(fd, ring.at(s), m, pos + off, host_threads()))
            return fail(XS_ERR_IO, "%s: short read", path);
        HIPCHK(emit(off, m, ring.at(s)));
        HIPCHK(hipEventRecord(ring.ev[s], b->stream));
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    return XS_OK;
}

// nbytes of `path` from byte `pos` to the device at dst, on b->stream (synchronised on return)
int stream_file_to_device(xs_bank* b, const char* path, uint64_t pos, uint64_t nbytes, uint8_t* dst) {
    return stream_file(b, path, pos, nbytes, kLoadPiece, [&](uint64_t off, uint64_t m, const uint8_t* src) {
        return hipMemcpyAsync(dst + off, src, m, hipMemcpyHostToDevice, b->stream);
    });
}

// [off, off + n) of fd from src, split over up to `threads` threads; false on a write error
bool pwrite_all(int fd, const uint8_t* src, uint64_t n, uint64_t off, int threads) {
    auto run = [=](uint64_t a, uint64_t e, bool* ok) {
        while (a < e) {
            const ssize_t put = pwrite(fd, src + a, (size_t)(e - a), (off_t)(off + a));
            if (put <= 0) {
                if (put < 0 && errno == EINTR) continue;
                *ok = false;
                return;
            }
            a += (uint64_t)put;
        }
        *ok = true;
    };
    return par_io(n, threads, run);
}

// nbytes of the device buffer src to `path` from byte `pos` (the header before it is
// already written): pieces come back by DMA into a ring of pinned slots and are written
// by up to 8 threads while the next pieces cross
int stream_device_to_file(xs_bank* b, const char* path, uint64_t pos, uint64_t nbytes, const uint8_t* src) {
    const int fd = ::open(path, O_WRONLY | O_CLOEXEC);
    if (fd < 0) return fail(XS_ERR_IO, "cannot open %s for writing", path);
    FdCloser closer{fd};  // an error path's close; the success path closes (and checks) below
    PinnedRing ring{b->stream};
    const uint64_t piece = std::min<uint64_t>(kLoadPiece, std::max<uint64_t>(nbytes, 1));
    if (int rc = ring.init(piece)) return rc;
    const uint64_t pieces = (nbytes + piece - 1) / piece;
    auto queue = [&](uint64_t i) -> hipError_t {
        const int s = (int)(i % kLoadSlots);
        const uint64_t off = i * piece, m = std::min(piece, nbytes - off);
        hipError_t e = hipMemcpyAsync(ring.at(s), src + off, m, hipMemcpyDeviceToHost, b->stream);
        return e == hipSuccess ? hipEventRecord(ring.ev[s], b->stream) : e;
    };
    for (uint64_t i = 0; i < std::min<uint64_t>(pieces, kLoadSlots); ++i) HIPCHK(queue(i));
    for (uint64_t i = 0; i < pieces; ++i) {
        const int s = (int)(i % kLoadSlots);
        HIPCHK(hipEventSynchronize(ring.ev[s]));
        const uint64_t off = i * piece, m = std::min(piece, nbytes - off);
        if (!pwrite_all(fd, ring.at(s), m, pos + off, host_threads()))
            return fail(XS_ERR_IO, "write to %s failed", path);
        if (i + kLoadSlots < pieces) HIPCHK(queue(i + kLoadSlots));
    }
    closer.fd = -1;
    if (::close(fd) != 0) return fail(XS_ERR_IO, "write to %s failed: %s", path, strerror(errno));
    return XS_OK;
}

// The bank's payload in file layout to `path` from byte `pos`.
int write_file_payload(xs_bank* b, const char* path, uint64_t pos) {
    const uint64_t nbytes = b->payload_bytes();
    HIPCHK(hipSetDevice(b->device));
    if (int rc = ws_enter(b, b->stream)) return rc;
    if (b->kind == XS_BANK_RBLOOM || b->pitch == b->page)
        return stream_device_to_file(b, path, pos, nbytes, b->image.as<uint8_t>());
    if (int rc = b->tmp.ensure(nbytes)) return rc;
    HIPCHK(launch_repack(b->image.as<uint8_t>(), b->pitch, b->tmp.as<uint8_t>(), b->page, b->sig_total(), b->page,
                         b->stream));
    return stream_device_to_file(b, path, pos, nbytes, b->tmp.as<uint8_t>());
}

// The bank's payload (the file's bytes after the header, at `pos`) into its image.
int upload_file_payload(xs_bank* b, const char* path, uint64_t pos) {
    const uint64_t nbytes = b->payload_bytes();
    HIPCHK(hipSetDevice(b->device));
    if (int rc = ws_enter(b, b->stream)) return rc;
    if (b->kind == XS_BANK_RBLOOM || b->pitch == b->page)
        return stream_file_to_device(b, path, pos, nbytes, b->image.as<uint8_t>());
    if (int rc = b->tmp.ensure(nbytes)) return rc;
    if (int rc = stream_file_to_device(b, path, pos, nbytes, b->tmp.as<uint8_t>())) return rc;
    HIPCHK(launch_repack(b->tmp.as<uint8_t>(), b->page, b->image.as<uint8_t>(), b->pitch, b->sig_total(), b->page,
                         b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    return XS_OK;
}

// ---- writers -----------------------------------------------------------------
template <class T>
void put(std::ofstream& o, T v) {
    o.write(reinterpret_cast<const char*>(&v), sizeof(T));
}

int write_cobs_file(xs_bank* b, const char* path) {
    std::ofstream o(path, std::ios::binary | std::ios::trunc);
    if (!o) return fail(XS_ERR_IO, "cannot open %s for writing", path);
    o.write("COBS:", 5);
    if (b->kind == XS_BANK_COBS_CLASSIC) {
        o.write(kClassicMagic, (std::streamsize)strlen(kClassicMagic));
        put<uint32_t>(o, 1);
        put<uint32_t>(o, (uint32_t)b->D);
        put<uint32_t>(o, b->k);
        put<uint8_t>(o, (uint8_t)b->canonicalize);
        put<uint64_t>(o, b->sig[0]);
        put<uint64_t>(o, b->h);
        for (auto& n : b->names) o << n << '\n';
        o.write(kClassicMagic, (std::streamsize)strlen(kClassicMagic));
    } else {
        o.write(kCompactMagic, (std::streamsize)strlen(kCompactMagic));
        put<uint32_t>(o, 1);
        put<uint32_t>(o, b->k);
        put<uint8_t>(o, (uint8_t)b->canonicalize);
        put<uint64_t>(o, b->G);
        for (uint64_t g = 0; g < b->G; ++g) {
            put<uint64_t>(o, b->sig[g]);
            put<uint64_t>(o, b->h);
        }
        put<uint64_t>(o, b->page);
        put<uint32_t>(o, (uint32_t)b->D);
        for (auto& n : b->names) o << n << '\n';
        o.write(kCompactMagic, (std::streamsize)strlen(kCompactMagic));
        const uint64_t pos = (uint64_t)o.tellp();
        const uint64_t pad = (b->page - pos % b->page) % b->page;
        std::vector<char> z(pad, 0);
        o.write(z.data(), (std::streamsize)pad);
    }
    const uint64_t pos = (uint64_t)o.tellp();
    o.close();
    if (!o) return fail(XS_ERR_IO, "write to %s failed", path);
    return write_file_payload(b, path, pos);  // the payload after the header, streamed from the device
}

int write_bloom_file(xs_bank* b, const char* path) {
    std::ofstream o(path, std::ios::binary | std::ios::trunc);
    if (!o) return fail(XS_ERR_IO, "cannot open %s for writing", path);
    put<uint64_t>(o, b->h);
    o.close();
    if (!o) return fail(XS_ERR_IO, "write to %s failed", path);
    return write_file_payload(b, path, 8);
}

}  // namespace

extern "C" {

// a handle that fails on its way drops through its destructor; *out takes it only on success
int xs_bank_open(const char* path, int kind, int device, xs_bank** out) {
    return xs::guard([&]() -> int {
        if (!path || !out) return fail(XS_ERR_ARG, "null argument");
        *out = nullptr;
        if (kind != XS_BANK_COBS_CLASSIC && kind != XS_BANK_COBS_COMPACT && kind != XS_BANK_RBLOOM)
            return fail(XS_ERR_ARG, "unknown bank kind %d", kind);
        BankGeometry g;
        if (int rc = read_checked_header(path, kind, &g)) return rc;  // before any HIP call
        if (kind != XS_BANK_RBLOOM)
            if (int rc = check_lds_budget(g.D, path)) return rc;
        auto b = bank_of(device, g);
        if (int rc = alloc_image(b.get())) return rc;
        if (int rc = upload_file_payload(b.get(), path, g.payload_offset)) return rc;
        *out = b.release();
        return XS_OK;
    });
}

int xs_bank_file_info(const char* path, int kind, xs_bank_info_t* out, uint64_t* payload_offset) {
    return xs::guard([&]() -> int {
        if (!path || !out) return fail(XS_ERR_ARG, "null argument");
        memset(out, 0, sizeof(*out));
        if (payload_offset) *payload_offset = 0;
        if (kind != XS_BANK_COBS_CLASSIC && kind != XS_BANK_COBS_COMPACT && kind != XS_BANK_RBLOOM)
            return fail(XS_ERR_ARG, "unknown bank kind %d", kind);
        BankGeometry g;
        if (int rc = read_checked_header(path, kind, &g)) return rc;
        out->kind = kind;
        out->device = -1;
        out->term_size = g.k;
        out->num_hashes = (uint32_t)g.h;
        out->canonicalize = g.canonicalize;
        out->num_docs = g.D;
        out->num_groups = kind == XS_BANK_RBLOOM ? 0 : g.G;
        out->page_size = g.page;
        out->signature_rows = g.sig_total;
        out->bloom_bits = kind == XS_BANK_RBLOOM ? g.nbytes * 8 : 0;
        out->device_bytes = g.dev_bytes;
        out->device_row_pitch = g.pitch;
        if (payload_offset) *payload_offset = g.payload_offset;
        return XS_OK;
    });
}

int xs_bank_file_names(const char* path, int kind, char* buf, uint64_t cap, uint64_t* bytes) {
    return xs::guard([&]() -> int {
        if (!path || !bytes || (cap && !buf)) return fail(XS_ERR_ARG, "null argument");
        *bytes = 0;
        if (kind != XS_BANK_COBS_CLASSIC && kind != XS_BANK_COBS_COMPACT && kind != XS_BANK_RBLOOM)
            return fail(XS_ERR_ARG, "unknown bank kind %d", kind);
        BankGeometry g;
        if (int rc = read_checked_header(path, kind, &g)) return rc;
        uint64_t need = 0;
        for (auto& n : g.names) need += n.size() + 1;
        *bytes = need;
        if (need > cap) return XS_OK;  // the caller asks again with room for *bytes
        for (auto& n : g.names) {
            memcpy(buf, n.data(), n.size());
            buf[n.size()] = '\n';
            buf += n.size() + 1;
        }
        return XS_OK;
    });
}

int xs_bank_open_docs(const char* path, int device, uint64_t doc_lo, uint64_t doc_hi, xs_bank** out) {
    return xs::guard([&]() -> int {
        if (!path || !out) return fail(XS_ERR_ARG, "null argument");
        *out = nullptr;
        // the whole file's header, payload size included, as xs_bank_file_info checks it; only the slice has to
        // meet the LDS budget (the split exists for banks of more docs than one handle takes)
        BankGeometry full;
        std::string err;
        if (int rc = read_checked_header(path, XS_BANK_COBS_CLASSIC, &full)) return rc;
        const uint64_t D = full.D, R = full.page, S = full.sig[0], pos = full.payload_offset;
        if (doc_lo % 8 || doc_lo >= doc_hi || doc_hi > D || (doc_hi % 8 && doc_hi != D))
            return fail(XS_ERR_ARG, "doc range [%llu, %llu) of %llu docs: bounds must be multiples of 8 (or the end)",
                        (unsigned long long)doc_lo, (unsigned long long)doc_hi, (unsigned long long)D);
        BankGeometry g;
        g.kind = XS_BANK_COBS_CLASSIC;
        g.k = full.k;
        g.h = full.h;
        g.canonicalize = full.canonicalize;
        g.D = doc_hi - doc_lo;
        g.G = 1;
        g.page = (g.D + 7) / 8;
        g.sig.assign(1, S);
        g.names.assign(full.names.begin() + (ptrdiff_t)doc_lo, full.names.begin() + (ptrdiff_t)doc_hi);
        if (int rc = check_geometry(&g, GeometrySource::kFile, &err)) return refused(rc, path, err);
        if (int rc = check_lds_budget(g.D, path)) return rc;
        auto b = bank_of(device, g);
        if (int rc = alloc_image(b.get())) return rc;
        // whole rows to the device a piece at a time (about kLoadPiece bytes of whole rows), each
        // piece's byte columns [doc_lo / 8, + page) repacked into the image at its first row: the
        // device holds the slice and one piece of whole rows, never the whole bank (config 5's
        // column split exists for banks one GPU cannot hold)
        const uint64_t c0 = doc_lo / 8, P = b->page;
        const uint64_t piece = std::max<uint64_t>(1, kLoadPiece / R) * R;
        HIPCHK(hipSetDevice(b->device));
        if (int rc = ws_enter(b.get(), b->stream)) return rc;
        if (int rc = b->tmp.ensure(std::min<uint64_t>(piece, S * R))) return rc;
        uint8_t* stage = b->tmp.as<uint8_t>();
        // one staging buffer: the stream orders each piece's copy after the previous piece's repack
        if (int rc = stream_file(b.get(), path, pos, S * R, piece, [&](uint64_t off, uint64_t m, const uint8_t* src) {
                hipError_t e = hipMemcpyAsync(stage, src, m, hipMemcpyHostToDevice, b->stream);
                if (e != hipSuccess) return e;
                return launch_repack(stage + c0, R, b->image.as<uint8_t>() + off / R * b->pitch, b->pitch, m / R, P,
                                     b->stream);
            }))
            return rc;
        b->tmp.release();  // the staging piece is not kept beside the slice
        *out = b.release();
        return XS_OK;
    });
}

int xs_bank_create_cobs(int device, int kind, uint32_t term_size, uint32_t num_hashes,
                        uint64_t num_docs, uint64_t page_size, uint64_t num_groups,
                        const uint64_t* sig, const char* const* doc_names, xs_bank** out) {
    return xs::guard([&]() -> int {
        if (!out || !sig) return fail(XS_ERR_ARG, "null argument");
        *out = nullptr;
        if (kind != XS_BANK_COBS_CLASSIC && kind != XS_BANK_COBS_COMPACT)
            return fail(XS_ERR_ARG, "kind must be a COBS kind");
        if (kind == XS_BANK_COBS_CLASSIC && (num_groups != 1 || page_size != num_docs / 8 + (num_docs % 8 != 0)))
            return fail(XS_ERR_ARG, "classic banks have one group of ceil(D/8) bytes");
        // the geometry is checked before sig's num_groups entries and the names are touched
        BankGeometry g;
        g.kind = kind;
        g.k = term_size;
        g.h = num_hashes;
        g.D = num_docs;
        g.G = num_groups;
        g.page = page_size;
        std::string err;
        if (int rc = check_term_and_hashes(g.k, g.h, &err)) return refused(rc, nullptr, err);
        if (int rc = check_cobs_shape(num_docs, num_groups, page_size, GeometrySource::kArguments, &err))
            return refused(rc, nullptr, err);
        if (int rc = check_lds_budget(num_docs, nullptr)) return rc;  // bounds the docs, and so the groups
        g.sig.assign(sig, sig + num_groups);
        if (int rc = check_geometry(&g, GeometrySource::kArguments, &err)) return refused(rc, nullptr, err);
        g.names.reserve((size_t)num_docs);
        for (uint64_t i = 0; i < num_docs; ++i) {
            if (doc_names && !doc_names[i]) return fail(XS_ERR_ARG, "doc_names[%llu] is NULL", (unsigned long long)i);
            g.names.push_back(doc_names ? std::string(doc_names[i]) : std::to_string(i));
        }
        auto b = bank_of(device, g);
        if (int rc = alloc_image(b.get())) return rc;
        *out = b.release();
        return XS_OK;
    });
}

int xs_bank_create_bloom(int device, uint32_t term_size, uint64_t nbytes, uint32_t nhash,
                         xs_bank** out) {
    return xs::guard([&]() -> int {
        if (!out) return fail(XS_ERR_ARG, "null argument");
        *out = nullptr;
        BankGeometry g;
        g.kind = XS_BANK_RBLOOM;
        g.k = term_size;
        g.h = nhash;
        g.nbytes = nbytes;
        g.D = 1;
        g.names.push_back("0");
        std::string err;
        if (int rc = check_geometry(&g, GeometrySource::kArguments, &err)) return refused(rc, nullptr, err);
        auto b = bank_of(device, g);
        if (int rc = alloc_image(b.get())) return rc;
        *out = b.release();
        return XS_OK;
    });
}

int xs_bank_save(xs_bank* b, const char* path) {
    return xs::guard([&]() -> int {
        if (!b || !path) return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(b->mu);
        HIPCHK(hipSetDevice(b->device));
        HIPCHK(hipDeviceSynchronize());
        // the file is written beside its destination and renamed over it once whole: a failed
        // save leaves no short or holed file at `path`, and an existing model there intact
        struct Partial {  // removed on every way out (an exception included) but the rename
            std::string path;
            bool renamed = false;
            ~Partial() {
                if (!renamed) (void)::unlink(path.c_str());
            }
        } tmp{std::string(path) + ".xs-part-" + std::to_string((long)getpid())};
        const char* t = tmp.path.c_str();
        if (int rc = b->kind == XS_BANK_RBLOOM ? write_bloom_file(b, t) : write_cobs_file(b, t)) return rc;
        if (::rename(t, path) != 0) return fail(XS_ERR_IO, "cannot rename %s to %s: %s", t, path, strerror(errno));
        tmp.renamed = true;
        return XS_OK;
    });
}

int xs_bank_download(xs_bank* b, void* host, uint64_t nbytes) {
    return xs::guard([&]() -> int {
        if (!b || !host) return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(b->mu);
        HIPCHK(hipSetDevice(b->device));
        HIPCHK(hipDeviceSynchronize());
        return download_payload(b, host, nbytes);
    });
}

int xs_bank_upload(xs_bank* b, const void* host, uint64_t nbytes) {
    return xs::guard([&]() -> int {
        if (!b || !host) return fail(XS_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(b->mu);
        return upload_payload(b, host, nbytes);
    });
}

}  // extern "C"
