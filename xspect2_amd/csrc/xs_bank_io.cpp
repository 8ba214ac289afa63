// xs_bank_io.cpp — bank files and device residency: the COBS / rbloom file formats, the device image, payloads
// streamed between files and the device through a ring of pinned slots, the open / create / save entry points.
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

#include "xs_host.h"

using namespace xs;

namespace {

const char kClassicMagic[] = "CLASSIC_INDEX";
const char kCompactMagic[] = "COMPACT_INDEX";

int validate_geometry(xs_bank* b) {
    if (b->k < 1 || b->k > kMaxK)
        return fail(XS_ERR_UNSUPPORTED, "term_size %u unsupported on the device (1..%u)", b->k, kMaxK);
    if (b->h < 1 || b->h > kMaxHashes)
        return fail(XS_ERR_UNSUPPORTED, "num_hashes %u unsupported on the device (1..%u)", b->h,
                    kMaxHashes);
    if (b->kind == XS_BANK_RBLOOM) {
        if (b->nbytes == 0) return fail(XS_ERR_FORMAT, "empty rbloom filter");
        return XS_OK;
    }
    if (b->D == 0) return fail(XS_ERR_FORMAT, "bank has no documents");
    if (b->page == 0 || b->G == 0 || b->sig.size() != b->G)
        return fail(XS_ERR_FORMAT, "bad group geometry");
    if (b->G * 8 * b->page < b->D || (b->G - 1) * 8 * b->page >= b->D)
        return fail(XS_ERR_FORMAT, "groups (%llu x %llu bytes) do not match %llu docs",
                    (unsigned long long)b->G, (unsigned long long)b->page,
                    (unsigned long long)b->D);
    for (auto s : b->sig)
        if (s == 0) return fail(XS_ERR_FORMAT, "zero signature size");
    // Device row pitch: 16, 32, 64 or a multiple of 128 bytes, so that no row
    // straddles a 128-byte line (a 48-byte pitch made 2 rows in 8 cost two
    // line fills).  The kernels load only the (page + 15) / 16 data chunks.
    const uint64_t p16 = (b->page + 15) / 16 * 16;
    b->pitch = p16 <= 64 ? (p16 <= 16 ? 16 : p16 <= 32 ? 32 : 64) : (p16 + 127) / 128 * 128;
    int wpb;
    size_t lds;
    if (probe_blocks(b->D, &wpb, &lds) != 0)
        return fail(XS_ERR_UNSUPPORTED, "%llu documents exceed the LDS counter budget",
                    (unsigned long long)b->D);
    return XS_OK;
}

// Allocate the (zeroed) device image and group table.
int alloc_image(xs_bank* b) {
    HIPCHK(hipSetDevice(b->device));
    if (!b->stream) HIPCHK(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
    b->dev_bytes = b->kind == XS_BANK_RBLOOM ? (b->nbytes + 15) / 16 * 16 + 16 : b->sig_total() * b->pitch;
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

// ---- little binary reader -------------------------------------------------
struct Reader {
    std::ifstream f;
    bool ok = true;
    uint64_t fsize = 0;
    bool open(const char* path) {  // false: `path` cannot be opened
        f.open(path, std::ios::binary);
        if (!f) return false;
        f.seekg(0, std::ios::end);
        fsize = (uint64_t)f.tellg();
        f.seekg(0);
        return true;
    }
    template <class T>
    T get() {
        T v{};
        f.read(reinterpret_cast<char*>(&v), sizeof(T));
        if (!f) ok = false;
        return v;
    }
    bool expect(const char* s) {
        std::string got(strlen(s), '\0');
        f.read(&got[0], (std::streamsize)got.size());
        if (!f || got != s) ok = false;
        return ok;
    }
    std::string line() {
        std::string s;
        if (!std::getline(f, s)) ok = false;
        return s;
    }
};

template <class T>
void put(std::ofstream& o, T v) {
    o.write(reinterpret_cast<const char*>(&v), sizeof(T));
}

int read_cobs_header(xs_bank* b, Reader& rd, const char* path) {
    if (!rd.expect("COBS:")) return fail(XS_ERR_FORMAT, "%s: not a COBS index", path);
    if (b->kind == XS_BANK_COBS_CLASSIC) {
        if (!rd.expect(kClassicMagic)) return fail(XS_ERR_FORMAT, "%s: not a classic index", path);
        const uint32_t ver = rd.get<uint32_t>();
        const uint32_t nd = rd.get<uint32_t>();
        b->k = rd.get<uint32_t>();
        b->canonicalize = rd.get<uint8_t>();
        const uint64_t s = rd.get<uint64_t>();
        b->h = (uint32_t)rd.get<uint64_t>();
        if (!rd.ok || ver != 1) return fail(XS_ERR_FORMAT, "%s: bad classic header", path);
        b->D = nd;
        b->G = 1;
        b->page = (nd + 7) / 8;
        b->sig.assign(1, s);
        for (uint32_t i = 0; i < nd; ++i) b->names.push_back(rd.line());
        if (!rd.expect(kClassicMagic)) return fail(XS_ERR_FORMAT, "%s: bad classic trailer", path);
    } else {
        if (!rd.expect(kCompactMagic)) return fail(XS_ERR_FORMAT, "%s: not a compact index", path);
        const uint32_t ver = rd.get<uint32_t>();
        b->k = rd.get<uint32_t>();
        b->canonicalize = rd.get<uint8_t>();
        const uint64_t G = rd.get<uint64_t>();
        if (!rd.ok || ver != 1 || G == 0 || G > (1u << 20))
            return fail(XS_ERR_FORMAT, "%s: bad compact header", path);
        b->G = G;
        for (uint64_t g = 0; g < G; ++g) {
            b->sig.push_back(rd.get<uint64_t>());
            const uint32_t hg = (uint32_t)rd.get<uint64_t>();
            if (g == 0) b->h = hg;
            else if (hg != b->h) return fail(XS_ERR_FORMAT, "%s: mixed num_hashes", path);
        }
        b->page = rd.get<uint64_t>();
        const uint32_t nd = rd.get<uint32_t>();
        b->D = nd;
        for (uint32_t i = 0; i < nd; ++i) b->names.push_back(rd.line());
        if (!rd.expect(kCompactMagic)) return fail(XS_ERR_FORMAT, "%s: bad compact trailer", path);
        if (b->page == 0) return fail(XS_ERR_FORMAT, "%s: zero page size", path);
        const uint64_t pos = (uint64_t)rd.f.tellg();
        const uint64_t pad = (b->page - pos % b->page) % b->page;
        rd.f.seekg((std::streamoff)(pos + pad));
    }
    if (!rd.ok) return fail(XS_ERR_FORMAT, "%s: truncated header", path);
    if (b->canonicalize != 1)
        return fail(XS_ERR_UNSUPPORTED, "%s: non-canonical COBS indices are not supported", path);
    return XS_OK;
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
        Reader rd;
        if (!rd.open(path)) return fail(XS_ERR_IO, "cannot open %s", path);
        auto b = std::make_unique<xs_bank>(device, kind);
        if (kind == XS_BANK_RBLOOM) {
            b->h = (uint32_t)rd.get<uint64_t>();
            if (!rd.ok || rd.fsize <= 8) return fail(XS_ERR_FORMAT, "%s: truncated rbloom file", path);
            b->nbytes = rd.fsize - 8;
            b->D = 1;
            b->names.push_back("0");
            // An rbloom file carries no k (the model JSON does); default to XspecT's
            // k = 21 (train.py:167-174) until xs_bank_set_term_size overrides it.
            b->k = 21;
        } else if (int rc = read_cobs_header(b.get(), rd, path)) {
            return rc;
        }
        if (int rc = validate_geometry(b.get())) return rc;
        const uint64_t pos = (uint64_t)rd.f.tellg();
        if (rd.fsize - pos != b->payload_bytes())
            return fail(XS_ERR_FORMAT, "%s: payload is %llu bytes, header implies %llu", path,
                        (unsigned long long)(rd.fsize - pos), (unsigned long long)b->payload_bytes());
        if (int rc = alloc_image(b.get())) return rc;
        if (int rc = upload_file_payload(b.get(), path, pos)) return rc;
        *out = b.release();
        return XS_OK;
    });
}

int xs_bank_open_docs(const char* path, int device, uint64_t doc_lo, uint64_t doc_hi, xs_bank** out) {
    return xs::guard([&]() -> int {
        if (!path || !out) return fail(XS_ERR_ARG, "null argument");
        *out = nullptr;
        Reader rd;
        if (!rd.open(path)) return fail(XS_ERR_IO, "cannot open %s", path);
        auto full = std::make_unique<xs_bank>(device, XS_BANK_COBS_CLASSIC);
        if (int rc = read_cobs_header(full.get(), rd, path)) return rc;
        const uint64_t D = full->D, R = full->page, S = full->sig[0];
        if (doc_lo % 8 || doc_lo >= doc_hi || doc_hi > D || (doc_hi % 8 && doc_hi != D))
            return fail(XS_ERR_ARG, "doc range [%llu, %llu) of %llu docs: bounds must be multiples of 8 (or the end)",
                        (unsigned long long)doc_lo, (unsigned long long)doc_hi, (unsigned long long)D);
        const uint64_t pos = (uint64_t)rd.f.tellg();
        if (rd.fsize - pos != S * R)
            return fail(XS_ERR_FORMAT, "%s: payload is %llu bytes, header implies %llu", path,
                        (unsigned long long)(rd.fsize - pos), (unsigned long long)(S * R));
        auto b = std::make_unique<xs_bank>(device, XS_BANK_COBS_CLASSIC);
        b->k = full->k;
        b->h = full->h;
        b->canonicalize = full->canonicalize;
        b->D = doc_hi - doc_lo;
        b->G = 1;
        b->page = (b->D + 7) / 8;
        b->sig.assign(1, S);
        b->names.assign(full->names.begin() + (ptrdiff_t)doc_lo, full->names.begin() + (ptrdiff_t)doc_hi);
        if (int rc = validate_geometry(b.get())) return rc;
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
        if (kind == XS_BANK_COBS_CLASSIC && (num_groups != 1 || page_size != (num_docs + 7) / 8))
            return fail(XS_ERR_ARG, "classic banks have one group of ceil(D/8) bytes");
        auto b = std::make_unique<xs_bank>(device, kind);
        b->k = term_size;
        b->h = num_hashes;
        b->D = num_docs;
        b->G = num_groups;
        b->page = page_size;
        b->sig.assign(sig, sig + num_groups);
        for (uint64_t i = 0; i < num_docs; ++i)
            b->names.push_back(doc_names ? std::string(doc_names[i]) : std::to_string(i));
        if (int rc = validate_geometry(b.get())) return rc;
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
        auto b = std::make_unique<xs_bank>(device, XS_BANK_RBLOOM);
        b->k = term_size;
        b->h = nhash;
        b->nbytes = nbytes;
        b->D = 1;
        b->names.push_back("0");
        if (int rc = validate_geometry(b.get())) return rc;
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
