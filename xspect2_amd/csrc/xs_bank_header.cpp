// xs_bank_header.cpp — bank file headers and bank geometry on the host alone (xs_bank_header.h).
#include "xs_bank_header.h"

#include <cstring>
#include <fstream>

#include "../../include/xspect_hip.h"

namespace xs {
namespace {

const char kClassicMagic[] = "CLASSIC_INDEX";
const char kCompactMagic[] = "COMPACT_INDEX";

int refuse(int code, std::string* err, std::string msg) {
    if (err) *err = std::move(msg);
    return code;
}

std::string u64s(uint64_t v) { return std::to_string((unsigned long long)v); }

// a * b and a + b into *out; false when the value does not fit 64 bits
bool mul(uint64_t a, uint64_t b, uint64_t* out) { return !__builtin_mul_overflow(a, b, out); }
bool add(uint64_t a, uint64_t b, uint64_t* out) { return !__builtin_add_overflow(a, b, out); }

// v rounded up to a multiple of m (m > 0); false when that does not fit 64 bits
bool round_up(uint64_t v, uint64_t m, uint64_t* out) {
    uint64_t t;
    if (!add(v, m - 1, &t)) return false;
    *out = t / m * m;
    return true;
}

int overflow_code(GeometrySource src) { return src == GeometrySource::kFile ? XS_ERR_FORMAT : XS_ERR_ARG; }

// The file behind a header: every read is checked, and after the first one that fails nothing more is read.
struct Reader {
    std::ifstream f;
    bool ok = true;
    uint64_t fsize = 0;
    bool open(const char* path) {  // false: `path` cannot be opened
        f.open(path, std::ios::binary);
        if (!f) return false;
        f.seekg(0, std::ios::end);
        const std::streamoff end = f.tellg();
        if (end < 0) return false;
        fsize = (uint64_t)end;
        f.seekg(0);
        return (bool)f;
    }
    uint64_t pos() {
        if (!ok) return fsize;
        const std::streamoff p = f.tellg();
        if (p < 0) {
            ok = false;
            return fsize;
        }
        return (uint64_t)p;
    }
    uint64_t left() {  // bytes between the read position and the file's end
        const uint64_t p = pos();
        return p < fsize ? fsize - p : 0;
    }
    template <class T>
    T get() {
        T v{};
        if (!ok) return v;
        f.read(reinterpret_cast<char*>(&v), sizeof(T));
        if (!f) {
            ok = false;
            return T{};
        }
        return v;
    }
    bool expect(const char* s) {
        if (!ok) return false;
        std::string got(strlen(s), '\0');
        f.read(&got[0], (std::streamsize)got.size());
        if (!f || got != s) ok = false;
        return ok;
    }
    // one name: the bytes up to its '\n'; a name the file's end cuts off is a failed read
    bool line(std::string* s) {
        if (!ok) return false;
        if (!std::getline(f, *s) || f.eof()) ok = false;
        return ok;
    }
};

// num_docs names, each ending in '\n'.  A name takes at least its '\n', so more names than bytes left is
// refused before one is read, and the loop ends at the first failed read.
bool read_names(Reader& rd, uint64_t nd, std::vector<std::string>* names) {
    if (nd > rd.left()) return false;
    names->reserve((size_t)nd);
    std::string s;
    for (uint64_t i = 0; i < nd; ++i) {
        if (!rd.line(&s)) return false;
        names->push_back(s);
    }
    return true;
}

int read_cobs_header(BankGeometry* g, Reader& rd, std::string* err) {
    if (!rd.expect("COBS:")) return refuse(XS_ERR_FORMAT, err, "not a COBS index");
    if (g->kind == XS_BANK_COBS_CLASSIC) {
        if (!rd.expect(kClassicMagic)) return refuse(XS_ERR_FORMAT, err, "not a classic index");
        const uint32_t ver = rd.get<uint32_t>();
        const uint32_t nd = rd.get<uint32_t>();
        g->k = rd.get<uint32_t>();
        g->canonicalize = rd.get<uint8_t>();
        const uint64_t s = rd.get<uint64_t>();
        g->h = rd.get<uint64_t>();
        if (!rd.ok || ver != 1) return refuse(XS_ERR_FORMAT, err, "bad classic header");
        g->D = nd;
        g->G = 1;
        g->page = ((uint64_t)nd + 7) / 8;
        g->sig.assign(1, s);
        if (!read_names(rd, nd, &g->names))
            return refuse(XS_ERR_FORMAT, err, "the file does not hold the header's " + u64s(nd) + " doc names");
        if (!rd.expect(kClassicMagic)) return refuse(XS_ERR_FORMAT, err, "bad classic trailer");
        g->payload_offset = rd.pos();
    } else {
        if (!rd.expect(kCompactMagic)) return refuse(XS_ERR_FORMAT, err, "not a compact index");
        const uint32_t ver = rd.get<uint32_t>();
        g->k = rd.get<uint32_t>();
        g->canonicalize = rd.get<uint8_t>();
        const uint64_t G = rd.get<uint64_t>();
        // a group takes 16 header bytes: more groups than the file can hold are refused before one is read
        if (!rd.ok || ver != 1 || G == 0 || G > kHeaderMaxGroups || G > rd.left() / 16)
            return refuse(XS_ERR_FORMAT, err, "bad compact header");
        g->G = G;
        g->sig.reserve((size_t)G);
        for (uint64_t i = 0; i < G; ++i) {
            g->sig.push_back(rd.get<uint64_t>());
            const uint64_t hg = rd.get<uint64_t>();
            if (!rd.ok) return refuse(XS_ERR_FORMAT, err, "truncated header");
            if (i == 0) g->h = hg;
            else if (hg != g->h) return refuse(XS_ERR_FORMAT, err, "mixed num_hashes");
        }
        g->page = rd.get<uint64_t>();
        const uint32_t nd = rd.get<uint32_t>();
        if (!rd.ok) return refuse(XS_ERR_FORMAT, err, "truncated header");
        g->D = nd;
        if (!read_names(rd, nd, &g->names))
            return refuse(XS_ERR_FORMAT, err, "the file does not hold the header's " + u64s(nd) + " doc names");
        if (!rd.expect(kCompactMagic)) return refuse(XS_ERR_FORMAT, err, "bad compact trailer");
        if (g->page == 0) return refuse(XS_ERR_FORMAT, err, "zero page size");
        // the payload starts at the next multiple of the page size
        const uint64_t pos = rd.pos();
        if (!rd.ok || !round_up(pos, g->page, &g->payload_offset) || g->payload_offset > rd.fsize)
            return refuse(XS_ERR_FORMAT, err, "the padding after the header runs past the file's end");
    }
    if (!rd.ok) return refuse(XS_ERR_FORMAT, err, "truncated header");
    if (g->canonicalize != 1) return refuse(XS_ERR_UNSUPPORTED, err, "non-canonical COBS indices are not supported");
    return XS_OK;
}

}  // namespace

int check_cobs_shape(uint64_t D, uint64_t G, uint64_t page, GeometrySource src, std::string* err) {
    if (D == 0) return refuse(XS_ERR_FORMAT, err, "bank has no documents");
    if (page == 0 || G == 0) return refuse(XS_ERR_FORMAT, err, "bad group geometry");
    uint64_t group_docs, all_docs;
    if (!mul(page, 8, &group_docs) || !mul(G, group_docs, &all_docs))
        return refuse(overflow_code(src), err,
                      u64s(G) + " groups of " + u64s(page) + " bytes: the doc count does not fit 64 bits");
    // (G - 1) * group_docs cannot overflow once G * group_docs did not
    if (all_docs < D || (G - 1) * group_docs >= D)
        return refuse(XS_ERR_FORMAT, err,
                      "groups (" + u64s(G) + " x " + u64s(page) + " bytes) do not match " + u64s(D) + " docs");
    return XS_OK;
}

int check_term_and_hashes(uint32_t k, uint64_t h, std::string* err) {
    if (k < 1 || k > kHeaderMaxK)
        return refuse(XS_ERR_UNSUPPORTED, err,
                      "term_size " + u64s(k) + " unsupported on the device (1.." + u64s(kHeaderMaxK) + ")");
    if (h < 1 || h > kHeaderMaxHashes)
        return refuse(XS_ERR_UNSUPPORTED, err,
                      "num_hashes " + u64s(h) + " unsupported on the device (1.." + u64s(kHeaderMaxHashes) + ")");
    return XS_OK;
}

int check_geometry(BankGeometry* g, GeometrySource src, std::string* err) {
    if (int rc = check_term_and_hashes(g->k, g->h, err)) return rc;
    const int big = overflow_code(src);
    if (g->kind == XS_BANK_RBLOOM) {
        if (g->nbytes == 0) return refuse(XS_ERR_FORMAT, err, "empty rbloom filter");
        uint64_t bits, padded;
        // the filter's bit count, and the image: the bytes padded to 16 and one spare chunk
        if (!mul(g->nbytes, 8, &bits) || !round_up(g->nbytes, 16, &padded) || !add(padded, 16, &g->dev_bytes))
            return refuse(big, err, "an rbloom filter of " + u64s(g->nbytes) + " bytes does not fit 64 bits of bit index");
        g->sig_total = 0;
        g->pitch = 0;
        g->payload_bytes = g->nbytes;
        return XS_OK;
    }
    if (int rc = check_cobs_shape(g->D, g->G, g->page, src, err)) return rc;
    if (g->sig.size() != g->G) return refuse(XS_ERR_FORMAT, err, "bad group geometry");
    uint64_t total = 0;
    for (uint64_t s : g->sig) {
        if (s == 0) return refuse(XS_ERR_FORMAT, err, "zero signature size");
        if (!add(total, s, &total)) return refuse(big, err, "the signature sizes' sum does not fit 64 bits");
    }
    // Device row pitch: 16, 32, 64 or a multiple of 128 bytes, so that no row
    // straddles a 128-byte line (a 48-byte pitch made 2 rows in 8 cost two
    // line fills).  The kernels load only the (page + 15) / 16 data chunks.
    uint64_t p16;
    if (!round_up(g->page, 16, &p16)) return refuse(big, err, "page size " + u64s(g->page) + " does not fit a row pitch");
    if (p16 <= 64) g->pitch = p16 <= 16 ? 16 : p16 <= 32 ? 32 : 64;
    else if (!round_up(p16, 128, &g->pitch))
        return refuse(big, err, "page size " + u64s(g->page) + " does not fit a row pitch");
    g->sig_total = total;
    if (!mul(total, g->page, &g->payload_bytes) || !mul(total, g->pitch, &g->dev_bytes))
        return refuse(big, err,
                      u64s(total) + " signature rows of " + u64s(g->page) + " bytes do not fit 64 bits");
    return XS_OK;
}

int read_bank_header(const char* path, int kind, BankGeometry* g, std::string* err) {
    *g = BankGeometry{};
    g->kind = kind;
    Reader rd;
    if (!rd.open(path)) return refuse(XS_ERR_IO, err, "cannot open the file");
    if (kind == XS_BANK_RBLOOM) {
        g->h = rd.get<uint64_t>();
        if (!rd.ok || rd.fsize <= 8) return refuse(XS_ERR_FORMAT, err, "truncated rbloom file");
        g->nbytes = rd.fsize - 8;
        g->payload_offset = 8;
        g->D = 1;
        g->names.push_back("0");
        // An rbloom file carries no k (the model JSON does); default to XspecT's
        // k = 21 (train.py:167-174) until xs_bank_set_term_size overrides it.
        g->k = 21;
    } else if (int rc = read_cobs_header(g, rd, err)) {
        return rc;
    }
    if (int rc = check_geometry(g, GeometrySource::kFile, err)) return rc;
    // payload_offset <= fsize holds for every kind here
    if (rd.fsize - g->payload_offset != g->payload_bytes)
        return refuse(XS_ERR_FORMAT, err,
                      "payload is " + u64s(rd.fsize - g->payload_offset) + " bytes, header implies " +
                          u64s(g->payload_bytes));
    return XS_OK;
}

}  // namespace xs
