// Host-side sanitizer run (AddressSanitizer + UndefinedBehaviorSanitizer, host
// code only) of the FASTA/FASTQ reader and the JSON/FASTA writers of
// libxspect_hip.so: randomised well-formed and malformed inputs, every batch
// size from one byte up, 1..8 parser threads.  Functional equality with
// Biopython / json.dumps is tested in tests/test_fastx.py and
// tests/test_json_writer.py; this driver looks for memory errors only.  It also drives the host's plan
// of a contig typing call (xs_mlst_plan.h) over randomised record lengths and checks its invariants, and the
// bank file header reader (xs_bank_header.h) over truncations, bit flips, field edges and random splices of
// five small valid files: every case must end in a return code.
//   make -C tools/asan run
#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/xspect_hip.h"
#include "../../xspect2_amd/csrc/xs_bank_header.h"
#include "../../xspect2_amd/csrc/xs_internal.h"
#include "../../xspect2_amd/csrc/xs_mlst_plan.h"

namespace xs {
int set_error(int code, const char* msg) {  // the library's version lives in xs_api.cpp (GPU side)
    (void)msg;
    return code;
}
int fail(int code, const char* fmt, ...) {  // likewise
    (void)fmt;
    return code;
}
// likewise (xs_api.cpp pins host memory; no GPU here, so plain host memory)
int pinned_alloc(size_t bytes, void** out) {
    *out = malloc(bytes ? bytes : 1);
    return *out ? 0 : -6;
}
void pinned_free(void* p) { free(p); }
}  // namespace xs
extern "C" const char* xs_last_error(void) { return ""; }  // likewise

static std::mt19937_64 rng(12345);

static std::string rand_seq(size_t n, const char* alpha) {
    std::string s;
    const size_t m = strlen(alpha);
    for (size_t i = 0; i < n; ++i) s += alpha[rng() % m];
    return s;
}

static std::string make_fasta(int recs, bool crlf, bool trailing_nl) {
    std::string out, nl = crlf ? "\r\n" : "\n";
    for (int r = 0; r < recs; ++r) {
        out += ">r" + std::to_string(r) + (rng() % 2 ? " desc words\t x" : "") + nl;
        const size_t len = rng() % 400;
        const std::string s = rand_seq(len, "ACGTNacgtRY");
        const size_t w = 1 + rng() % 90;
        for (size_t i = 0; i < s.size(); i += w) out += s.substr(i, w) + nl;
        if (rng() % 7 == 0) out += nl;  // blank line
    }
    if (!trailing_nl && !out.empty()) out.resize(out.size() - nl.size());
    return out;
}

static std::string make_fastq(int recs, bool wrapped, bool trailing_nl, bool malformed) {
    std::string out;
    for (int r = 0; r < recs; ++r) {
        const size_t len = rng() % 300;
        const std::string s = rand_seq(len, "ACGTN");
        std::string q = rand_seq(len, "@+IJ#!");  // '@' and '+' in qualities
        if (malformed && r == recs / 2) q.resize(q.size() / 2);
        out += "@r" + std::to_string(r) + " x\n";
        if (wrapped && len > 10) out += s.substr(0, len / 2) + "\n" + s.substr(len / 2) + "\n";
        else out += s + "\n";
        out += "+\n";
        if (wrapped && q.size() > 10) out += q.substr(0, q.size() / 2) + "\n" + q.substr(q.size() / 2) + "\n";
        else out += q + "\n";
    }
    if (!trailing_nl && !out.empty()) out.pop_back();
    return out;
}

static int read_all(const std::string& path, int fmt, int threads, uint64_t batch, uint64_t* recs,
                    uint32_t part = 0, uint32_t parts = 1) {
    xs_fastx* r = nullptr;
    int rc = xs_fastx_open_range(path.c_str(), fmt, threads, 0, part, parts, &r);
    if (rc) return rc;
    *recs = 0;
    xs_fastx_batch b;
    for (;;) {
        rc = xs_fastx_next(r, batch, &b);
        if (rc || b.n == 0) break;
        *recs += b.n;
        // touch everything the batch hands out
        volatile uint64_t sink = 0;
        for (uint64_t i = 0; i < b.n; ++i) {
            for (uint64_t o = b.offsets[i]; o < b.offsets[i + 1]; ++o) sink += (uint8_t)b.seqs[o];
            for (uint64_t o = b.id_offsets[i]; o < b.id_offsets[i + 1]; ++o) sink += (uint8_t)b.ids[o];
            for (uint64_t o = b.desc_offsets[i]; o < b.desc_offsets[i + 1]; ++o) sink += (uint8_t)b.descs[o];
        }
        std::vector<uint32_t> idx;
        for (uint64_t i = 0; i < b.n; i += 2) idx.push_back((uint32_t)i);
        if (xs_write_fasta("/tmp/xs_asan_out.fasta", 0, b.seqs, b.offsets, b.descs, b.desc_offsets, idx.data(),
                           idx.size(), 60))
            return -99;
    }
    xs_fastx_close(r);
    return rc;
}

static void write_file(const std::string& path, const std::string& text) {
    FILE* f = fopen(path.c_str(), "wb");
    fwrite(text.data(), 1, text.size(), f);
    fclose(f);
}

// The plan of a contig typing call: record lengths around every threshold of the chunk rule and
// around the chunk widths, runs of short records between long ones, zero-length records; row and
// text caps from 1 up.  Returns the broken invariants; *plans counts the (lengths, width, caps) tried.
static int fuzz_mlst_plan(int* plans) {
    int bad = 0;
    auto expect = [&](bool ok, const char* what) {
        if (!ok && bad++ < 10) fprintf(stderr, "mlst plan: %s\n", what);
    };
    for (int trial = 0; trial < 300; ++trial) {
        const uint32_t k = (uint32_t[]){1, 7, 21, 31}[rng() % 4];
        xs_mlst_chunk_rule_t rule = xs::kReferenceRule;
        rule.long_len = k + rng() % 300;
        rule.scale10_len = rule.long_len + rng() % 1700;
        rule.scale100_len = rule.scale10_len + rng() % 4000;
        const uint64_t widths[3] = {k + rng() % 3, 2 * k + rng() % 100, 100 + rng() % 400};
        std::vector<uint64_t> special{0, k - 1, k, k + 1, rule.long_len - 1, rule.long_len, rule.long_len + 1,
                                      rule.scale10_len - 1, rule.scale10_len, rule.scale10_len + 1,
                                      rule.scale100_len - 1, rule.scale100_len, rule.scale100_len + 1};
        for (uint64_t w : widths)
            for (uint64_t W : {w, 10 * w, 100 * w})
                for (uint64_t n : {W - 1, W, W + 1, W + k - 2, W + k - 1, W + k, 2 * W, 2 * W - k + 1, 2 * W - k + 2})
                    special.push_back(n);
        // offsets: long records apart, in clusters, and between runs of short ones
        std::vector<uint64_t> ho{0};
        const int recs = (int)(rng() % 40);
        for (int r = 0; r < recs; ++r) {
            uint64_t len;
            switch (rng() % 4) {
                case 0: len = special[rng() % special.size()]; break;
                case 1: len = rng() % (rule.long_len + 1); break;  // mostly short
                case 2: len = rng() % (3 * rule.scale100_len + 1); break;
                default: len = 0;
            }
            ho.push_back(ho.back() + len);
        }
        const uint64_t n = ho.size() - 1;
        const xs::RecordKinds kinds = xs::classify_records(ho.data(), n, rule.long_len);
        {  // the long records and the short runs partition the records in order
            std::vector<int> seen(n, 0);
            uint64_t ns = 0, sb = 0;
            for (uint64_t r : kinds.longs) {
                expect(r < n && ho[r + 1] - ho[r] >= rule.long_len, "a long record is short");
                if (r < n) ++seen[r];
            }
            for (size_t i = 0; i < kinds.short_runs.size(); ++i) {
                const auto run = kinds.short_runs[i];
                expect(run.first < run.second && run.second <= n, "an empty or overlong short run");
                expect(i == 0 || kinds.short_runs[i - 1].second < run.first, "short runs touch or overlap");
                for (uint64_t r = run.first; r < run.second && r < n; ++r) {
                    expect(ho[r + 1] - ho[r] < rule.long_len, "a short record is long");
                    ++seen[r];
                    ++ns;
                    sb += ho[r + 1] - ho[r];
                }
            }
            for (int c : seen) expect(c == 1, "a record is in no kind or in two");
            expect(ns == kinds.n_short && sb == kinds.short_bytes, "short totals");
        }
        const uint64_t caps[][2] = {{1, 1}, {1, 1ull << 32}, {(1ull << 31) - 1, 1}, {2, 3}, {3, widths[2]},
                                    {1 + rng() % 50, 1 + rng() % 20000}, {(1ull << 31) - 1, 4ull << 30}};
        for (const auto& cap : caps) {
            const uint64_t row_cap = cap[0], text_cap = cap[1];
            std::vector<xs::MlstChunkRun> runs;
            std::vector<xs::ChunkRange> ranges;
            size_t first = 0;
            for (uint64_t w : widths) {  // locus after locus into the same arrays, as a call does
                xs::cut_chunk_ranges(kinds.longs, ho.data(), w, k, rule, row_cap, text_cap, &runs, &ranges);
                ++*plans;
                uint64_t want = 0;  // 1. the closed form xs_mlst_split_size returns
                for (uint64_t r : kinds.longs) {
                    const uint64_t len = ho[r + 1] - ho[r];
                    want += xs::mlst_rec_geom(len, xs::mlst_chunk_width(len, w, rule.scale10_len, rule.scale100_len), k)
                                .chunks;
                }
                uint64_t got = 0;
                for (size_t i = first; i < ranges.size(); ++i) {
                    const xs::ChunkRange& g = ranges[i];
                    expect(g.chunk_base == got, "chunk_base is not the running sum");                       // 5.
                    got += g.nc;
                    expect(g.nc >= 1 && g.nc <= row_cap, "a range's chunks outside 1 .. row_cap");          // 2.
                    expect(g.bytes <= text_cap || g.nc == 1, "a range of several chunks over text_cap");
                    expect(g.n_runs >= 1 && g.run0 + g.n_runs < runs.size(), "a range's runs out of the array");
                    if (g.run0 + g.n_runs >= runs.size()) continue;
                    const xs::MlstChunkRun* rr = runs.data() + g.run0;
                    expect(rr[0].row0 == 0 && rr[0].out == 0, "a range's first run does not start at 0");   // 3.
                    for (uint64_t j = 0; j < g.n_runs; ++j) {
                        expect(rr[j + 1].row0 > rr[j].row0 && rr[j + 1].out > rr[j].out, "row0 / byte0 not increasing");
                        const xs::MlstRecGeom geom = xs::mlst_rec_geom(rr[j].n, rr[j].W, k);
                        expect(rr[j].j0 + (rr[j + 1].row0 - rr[j].row0) <= geom.chunks, "a run past its record's chunks");
                        const uint64_t rec = rr[j].rec;
                        expect(rr[j].src == ho[rec] && rr[j].n == ho[rec + 1] - ho[rec], "a run's record");
                    }
                    expect(rr[g.n_runs].row0 == g.nc && rr[g.n_runs].out == g.bytes, "the sentinel's totals");
                    expect(g.carry_in == (i > first && ranges[i - 1].carry_out), "carry_in is not the last carry_out");
                    expect(g.carry_in == (rr[0].j0 > 0), "carry_in and the first run's j0 disagree");
                    if (i + 1 == ranges.size()) expect(!g.carry_out, "the last range carries out");
                }
                expect(got == want, "chunks over the ranges differ from the closed form");
                first = ranges.size();
            }
        }
    }
    return bad;
}

// Bank file headers (xs_bank_header.h): five valid files of the three layouts (the shapes of
// tests/test_bank_file_headers.py), and of each every truncation, every single-bit flip of the header (the
// fixed fields only where 1430 names make it 5.6 KB), every numeric field at its edge values and 2000 seeded
// random splices.  Every case ends in XS_OK or an error code; an accepted file's sizes multiply out exactly
// to the bytes it holds.  Then the argument side of check_geometry over sizes beyond 64 bits.  Returns the
// broken expectations; *cases counts the files read.
struct BankFile {
    int kind;
    std::string data;
    std::vector<std::pair<size_t, size_t>> fields;  // offset, width of every numeric field
    size_t header;                                  // bytes before the payload
    bool flip_fields_only;
};

template <class T>
static void put_le(std::string& s, T v) {
    s.append(reinterpret_cast<const char*>(&v), sizeof(T));
}

static BankFile classic_file(uint32_t docs, uint64_t sig) {
    BankFile f{XS_BANK_COBS_CLASSIC, "COBS:CLASSIC_INDEX", {{18, 4}, {22, 4}, {26, 4}, {30, 1}, {31, 8}, {39, 8}}, 0, false};
    put_le<uint32_t>(f.data, 1);
    put_le<uint32_t>(f.data, docs);
    put_le<uint32_t>(f.data, 21);
    put_le<uint8_t>(f.data, 1);
    put_le<uint64_t>(f.data, sig);
    put_le<uint64_t>(f.data, 7);
    for (uint32_t i = 0; i < docs; ++i) f.data += "d" + std::to_string(i) + "\n";
    f.data += "CLASSIC_INDEX";
    f.header = f.data.size();
    f.data += rand_seq(sig * ((docs + 7) / 8), "ACGT\n\x01\xff");
    return f;
}

static BankFile compact_file(uint32_t docs, std::vector<uint64_t> sig, uint64_t page, bool fields_only) {
    BankFile f{XS_BANK_COBS_COMPACT, "COBS:COMPACT_INDEX", {{18, 4}, {22, 4}, {26, 1}, {27, 8}}, 0, fields_only};
    put_le<uint32_t>(f.data, 1);
    put_le<uint32_t>(f.data, 31);
    put_le<uint8_t>(f.data, 1);
    put_le<uint64_t>(f.data, sig.size());
    uint64_t rows = 0;
    for (uint64_t s : sig) {
        f.fields.push_back({f.data.size(), 8});
        put_le<uint64_t>(f.data, s);
        f.fields.push_back({f.data.size(), 8});
        put_le<uint64_t>(f.data, 3);
        rows += s;
    }
    f.fields.push_back({f.data.size(), 8});
    put_le<uint64_t>(f.data, page);
    f.fields.push_back({f.data.size(), 4});
    put_le<uint32_t>(f.data, docs);
    for (uint32_t i = 0; i < docs; ++i) f.data += "a" + std::to_string(i) + "\n";
    f.data += "COMPACT_INDEX";
    f.data.append((page - f.data.size() % page) % page, '\0');
    f.header = f.data.size();
    f.data += rand_seq(rows * page, "ACGT\n\x01\xff");
    return f;
}

static int fuzz_bank_headers(int* cases, int* refused) {
    int bad = 0;
    const std::string path = "/tmp/xs_asan_bank.bin";
    auto read_one = [&](const BankFile& f, const std::string& data, int want /* 1 ok, 0 refused, -1 either */) {
        write_file(path, data);
        xs::BankGeometry g;
        std::string err;
        const int rc = xs::read_bank_header(path.c_str(), f.kind, &g, &err);
        ++*cases;
        if (rc) ++*refused;
        bool ok = rc == XS_OK || rc == XS_ERR_FORMAT || rc == XS_ERR_UNSUPPORTED;
        if (rc != XS_OK && err.empty()) ok = false;
        if (rc == XS_OK) {  // in 128 bits: the sizes multiply out to the bytes the file holds
            const unsigned __int128 rows = g.sig_total;
            unsigned __int128 sum = 0;
            for (uint64_t s : g.sig) sum += s;
            if (f.kind == XS_BANK_RBLOOM) ok = ok && g.payload_bytes == data.size() - 8 && g.dev_bytes >= g.nbytes + 16;
            else
                ok = ok && sum == rows && rows * g.page == data.size() - g.payload_offset &&
                     rows * g.pitch == g.dev_bytes && g.names.size() == g.D && g.sig.size() == g.G && g.h <= 16;
        }
        if (want >= 0 && (rc == XS_OK) != (want == 1)) ok = false;
        if (!ok && bad++ < 10) fprintf(stderr, "bank header: kind %d, %zu bytes: rc %d (%s)\n", f.kind, data.size(), rc, err.c_str());
    };
    std::vector<BankFile> files{classic_file(64, 257), classic_file(100, 101), compact_file(150, {37, 11, 23}, 8, false),
                                compact_file(1430, {5, 3, 4}, 64, true)};
    {
        BankFile r{XS_BANK_RBLOOM, std::string(), {{0, 8}}, 8, false};
        put_le<uint64_t>(r.data, 7);
        r.data += rand_seq(1000, "ACGT\n\x01\xff");
        files.push_back(r);
    }
    for (const BankFile& f : files) {
        read_one(f, f.data, 1);
        for (size_t n = 0; n < f.data.size(); ++n)  // an rbloom file carries no length: a cut past K is a smaller filter
            read_one(f, f.data.substr(0, n), f.kind == XS_BANK_RBLOOM ? (n > 8 ? 1 : 0) : 0);
        std::vector<size_t> flip;
        if (f.flip_fields_only) {
            for (auto fl : f.fields)
                for (size_t b = fl.first; b < fl.first + fl.second; ++b) flip.push_back(b);
        } else {
            for (size_t b = 0; b < f.header; ++b) flip.push_back(b);
        }
        for (size_t b : flip)
            for (int bit = 0; bit < 8; ++bit) {
                std::string d = f.data;
                d[b] = (char)(d[b] ^ (1 << bit));
                read_one(f, d, -1);
            }
        for (auto fl : f.fields) {
            uint64_t v = 0;
            memcpy(&v, f.data.data() + fl.first, fl.second);
            for (uint64_t nv : {uint64_t(0), uint64_t(1), v - 1, v + 1, uint64_t(1) << 31, (uint64_t(1) << 32) - 1,
                                (uint64_t(1) << 32) + v, (uint64_t(1) << 61) + v, uint64_t(1) << 63, ~uint64_t(0)}) {
                if (fl.second < 8 && nv >> (8 * fl.second)) continue;  // as far as the field is wide
                std::string d = f.data;
                memcpy(&d[fl.first], &nv, fl.second);
                read_one(f, d, -1);
            }
        }
        for (int trial = 0; trial < 400; ++trial) {  // splices: random bytes over the header, pieces cut out or doubled
            std::string d = f.data;
            const size_t at = rng() % (f.header + 1), n = 1 + rng() % 16;
            switch (rng() % 3) {
                case 0:
                    for (size_t i = at; i < std::min(d.size(), at + n); ++i) d[i] = (char)(rng() % 256);
                    break;
                case 1: d.erase(at, n); break;
                default: d.insert(at, d.substr(at, n));
            }
            read_one(f, d, -1);
        }
    }
    // arguments: sizes beyond 64 bits are XS_ERR_ARG, never a wrapped geometry
    auto args = [&](int kind, uint64_t D, uint64_t G, uint64_t page, std::vector<uint64_t> sig, uint64_t nbytes, int want) {
        xs::BankGeometry g;
        g.kind = kind;
        g.k = 21;
        g.h = 7;
        g.D = D;
        g.G = G;
        g.page = page;
        g.sig = sig;
        g.nbytes = nbytes;
        std::string err;
        const int rc = xs::check_geometry(&g, xs::GeometrySource::kArguments, &err);
        ++*cases;
        if (rc) ++*refused;
        if (rc != want && bad++ < 10) fprintf(stderr, "bank geometry: rc %d, expected %d (%s)\n", rc, want, err.c_str());
    };
    const uint64_t top = ~uint64_t(0);
    args(XS_BANK_COBS_CLASSIC, 64, 1, 8, {257}, 0, XS_OK);
    args(XS_BANK_COBS_CLASSIC, 64, 1, 8, {uint64_t(1) << 61}, 0, XS_ERR_ARG);
    args(XS_BANK_COBS_CLASSIC, 64, 1, 8, {uint64_t(1) << 60}, 0, XS_ERR_ARG);
    args(XS_BANK_COBS_COMPACT, 150, 3, 8, {uint64_t(1) << 63, uint64_t(1) << 63, 5}, 0, XS_ERR_ARG);
    args(XS_BANK_COBS_COMPACT, 150, uint64_t(1) << 61, 8, {5, 3, 4}, 0, XS_ERR_ARG);
    args(XS_BANK_COBS_COMPACT, 150, 3, uint64_t(1) << 61, {5, 3, 4}, 0, XS_ERR_ARG);
    args(XS_BANK_COBS_COMPACT, 150, top, top, {5, 3, 4}, 0, XS_ERR_ARG);
    args(XS_BANK_COBS_COMPACT, top, 1, top / 8 + 1, {5}, 0, XS_ERR_ARG);
    args(XS_BANK_COBS_COMPACT, 150, 2, 8, {5, 3}, 0, XS_ERR_FORMAT);
    args(XS_BANK_RBLOOM, 1, 0, 0, {}, 1000, XS_OK);
    args(XS_BANK_RBLOOM, 1, 0, 0, {}, uint64_t(1) << 61, XS_ERR_ARG);
    args(XS_BANK_RBLOOM, 1, 0, 0, {}, top, XS_ERR_ARG);
    args(XS_BANK_RBLOOM, 1, 0, 0, {}, 0, XS_ERR_FORMAT);
    return bad;
}

int main() {
    const std::string path = "/tmp/xs_asan_in.txt";
    int files = 0, errors = 0, unexpected = 0;
    auto sweep = [&](const std::string& text, int fmt, bool must_parse) {
        write_file(path, text);
        ++files;
        uint64_t whole = 0;
        for (uint64_t batch : {1ull, 7ull, 64ull, 1000ull, 1ull << 20})
            for (int threads : {1, 3, 8}) {
                uint64_t n = 0;
                const int rc = read_all(path, fmt, threads, batch, &n);
                if (rc) ++errors;  // malformed inputs must fail with an error code, not a crash
                if (rc && must_parse) ++unexpected;
                if (!rc) whole = n;
            }
        // byte-range parts (one rank each of a read-sharded job): well-formed
        // files split into parts whose record counts add up to the whole file's
        for (uint32_t parts : {2u, 3u, 7u}) {
            uint64_t sum = 0;
            bool failed = false;
            for (uint32_t part = 0; part < parts; ++part) {
                uint64_t n = 0;
                const int rc = read_all(path, fmt, 1 + part % 3, 64, &n, part, parts);
                if (rc) {
                    ++errors;
                    failed = true;
                }
                sum += n;
            }
            if (must_parse && (failed || sum != whole)) ++unexpected;
        }
    };
    for (int trial = 0; trial < 60; ++trial) {
        const bool fq = trial % 2;
        const int recs = (int)(rng() % 40);
        const bool bad = fq && trial % 11 == 0;
        const std::string text = fq ? make_fastq(recs, trial % 3 == 0, trial % 5 != 0, bad)
                                    : make_fasta(recs, trial % 3 == 0, trial % 5 != 0);
        sweep(text, fq ? XS_FASTX_FASTQ : XS_FASTX_FASTA, !bad);
        // the same file cut at a random byte, and with random bytes spliced in
        if (!text.empty()) {
            sweep(text.substr(0, rng() % text.size()), fq ? XS_FASTX_FASTQ : XS_FASTX_FASTA, !fq);
            std::string g = text;
            for (int i = 0; i < 8; ++i) g[rng() % g.size()] = (char)(rng() % 256);
            sweep(g, fq ? XS_FASTX_FASTQ : XS_FASTX_FASTA, false);
        }
    }
    for (const char* t : {"", ">", "@", ">\n", "@\n", "@r\n", "@r\nACGT\n+", "@r\nACGT\n+\nII", "\n\n\n", ">a\r\n\r\n",
                          "ACGT\n>x\nAC"})
        for (int fmt : {XS_FASTX_FASTA, XS_FASTX_FASTQ}) sweep(t, fmt, false);
    // JSON result sections: random hit matrices, masks, long ids
    for (int trial = 0; trial < 20; ++trial) {
        const uint64_t n = 1 + rng() % 300, D = 1 + rng() % 40;
        std::vector<uint32_t> hits(n * D);
        std::vector<uint64_t> nk(n);
        for (auto& h : hits) h = rng() % 200;
        for (auto& k : nk) k = 1 + rng() % 200;
        std::string ids, labels;
        std::vector<uint64_t> io{0}, lo{0};
        for (uint64_t i = 0; i < n; ++i) {
            ids += "\"read_" + std::to_string(i) + std::string(rng() % 30, 'x') + "\"";
            io.push_back(ids.size());
        }
        for (uint64_t d = 0; d < D; ++d) {
            labels += "\"" + std::to_string(470 + d) + "\"";
            lo.push_back(labels.size());
        }
        std::vector<uint8_t> mask(D);
        for (auto& m : mask) m = rng() % 3 != 0;
        FILE* f = fopen("/tmp/xs_asan_out.json", "wb");
        fclose(f);
        if (xs_write_result_sections("/tmp/xs_asan_out.json", n, D, hits.data(), 4, nk.data(), ids.c_str(), io.data(),
                                     labels.c_str(), lo.data(), trial % 2 ? mask.data() : nullptr, nullptr, 0,
                                     nullptr, 1 + trial % 8))
            ++errors;
    }
    // 128-bit id keys (xs_ids_hash128): ids of every length 0..200 packed back
    // to back in an exactly sized buffer, so a read past an id's end is caught
    for (int trial = 0; trial < 20; ++trial) {
        std::vector<uint64_t> off{0};
        std::string buf;
        for (int i = 0; i <= 200; ++i) {
            buf += rand_seq((size_t)((i + trial) % 201), "ACGT_:0123456789");
            off.push_back(buf.size());
        }
        std::vector<char> exact(buf.begin(), buf.end());
        std::vector<uint64_t> key(2 * (off.size() - 1));
        if (xs_ids_hash128(exact.data(), off.data(), off.size() - 1, key.data())) ++unexpected;
    }
    // a large batch takes the threaded path (n / 2^16 threads): keys equal the per-id ones;
    // a null offsets argument with ids is refused, not dereferenced
    {
        const uint64_t n = 300000;
        std::vector<uint64_t> off{0};
        std::string buf;
        for (uint64_t i = 0; i < n; ++i) {
            buf += "read_" + std::to_string(i);
            off.push_back(buf.size());
        }
        std::vector<char> exact(buf.begin(), buf.end());
        std::vector<uint64_t> key(2 * n), one(2);
        if (xs_ids_hash128(exact.data(), off.data(), n, key.data())) ++unexpected;
        for (uint64_t i = 0; i < n; i += 997) {
            const uint64_t o2[2] = {0, off[i + 1] - off[i]};
            if (xs_ids_hash128(exact.data() + off[i], o2, 1, one.data()) || one[0] != key[2 * i] ||
                one[1] != key[2 * i + 1])
                ++unexpected;
        }
        if (xs_ids_hash128(nullptr, nullptr, 5, key.data()) == 0) ++unexpected;
        else ++errors;
    }
    // member mask (xs_u64_member_mask): threaded pass over 400 k keys against sets with repeats,
    // 0 and 2^64-1, checked against std::set
    for (int trial = 0; trial < 6; ++trial) {
        const uint64_t n = 400000, m = trial == 0 ? 0 : 1000u * (uint64_t)trial;
        std::vector<uint64_t> keys(n), set;
        for (auto& k : keys) k = ((uint64_t)rng() << 32) ^ rng();
        keys[0] = 0;
        keys[1] = ~0ull;
        for (uint64_t j = 0; j < m; ++j) set.push_back(j % 2 ? keys[rng() % n] : ((uint64_t)rng() << 32) ^ rng());
        if (m) {
            set.push_back(0);
            set.push_back(~0ull);
            set.push_back(set[0]);
        }
        std::vector<uint8_t> out(n, 7);
        if (xs_u64_member_mask(keys.data(), n, set.empty() ? nullptr : set.data(), set.size(), out.data())) ++unexpected;
        std::set<uint64_t> ref(set.begin(), set.end());
        for (uint64_t i = 0; i < n; ++i)
            if (out[i] != (ref.count(keys[i]) ? 1 : 0)) ++unexpected;
    }
    // the persistent host workers (xs::parallel_for): 6 caller threads at once, each running jobs of
    // 1..20 tasks, some nested (a task starting its own job) and some throwing: every task runs
    // exactly once, a throwing task's exception reaches its caller after the others have finished
    {
        std::vector<std::thread> callers;
        std::atomic<int> bad{0};
        for (int c = 0; c < 6; ++c)
            callers.emplace_back([c, &bad] {
                std::mt19937_64 r(c);
                for (int job = 0; job < 300; ++job) {
                    const int n = 1 + (int)(r() % 20);
                    std::vector<std::atomic<int>> ran(n);
                    for (auto& x : ran) x = 0;
                    const int thrower = job % 7 == 0 ? (int)(r() % n) : -1;
                    bool caught = false;
                    try {
                        xs::parallel_for(n, [&](int t) {
                            ran[t]++;
                            if (job % 5 == 0) xs::parallel_for(3, [](int) {});  // nested
                            if (t == thrower) throw std::runtime_error("task failed");
                        });
                    } catch (const std::runtime_error&) {
                        caught = true;
                    }
                    if (caught != (thrower >= 0)) ++bad;
                    for (auto& x : ran)
                        if (x != 1) ++bad;
                }
            });
        for (auto& t : callers) t.join();
        unexpected += bad.load();
    }
    // repeated ids (xs_ids_has_duplicates): threaded passes over 300 k ids of 0..12 bytes, distinct
    // and with one repeat at random places, checked against std::set
    for (int trial = 0; trial < 6; ++trial) {
        const uint64_t n = 300000;
        std::vector<std::string> ids;
        std::set<std::string> seen;
        while (ids.size() < n) {
            std::string s = std::to_string(ids.size()) + rand_seq(rng() % 6, "ab:_");
            if (seen.insert(s).second) ids.push_back(s);
        }
        if (trial % 2) ids[rng() % n] = ids[rng() % n];
        std::string buf;
        std::vector<uint64_t> off{0};
        for (auto& s : ids) {
            buf += s;
            off.push_back(buf.size());
        }
        int dup = -1;
        if (xs_ids_has_duplicates(buf.data(), off.data(), n, &dup)) ++unexpected;
        const bool want = std::set<std::string>(ids.begin(), ids.end()).size() != n;
        if (dup != (want ? 1 : 0)) ++unexpected;
    }
    int plans = 0;
    unexpected += fuzz_mlst_plan(&plans);
    int bank_cases = 0, bank_refused = 0;
    unexpected += fuzz_bank_headers(&bank_cases, &bank_refused);
    printf("host sanitizer run: %d bank file headers and geometries (%d refused with a code); %d MLST contig plans; %d input files x 15 reader configurations + 12 byte-range parts, 20 JSON matrices, "
           "20 id-key batches + a threaded one, 6 member masks, 6 threaded repeat checks, 1800 worker-pool jobs from 6 threads (nested, throwing); %d clean error returns, "
           "%d unexpected results\n",
           bank_cases, bank_refused, plans, files, errors, unexpected);
    return unexpected ? 1 : 0;
}
