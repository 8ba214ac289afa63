// xs_fastx_parse.cpp — the host parser of the FASTA/FASTQ reader: line rules,
// record parsers, cut points, and a window's parallel parse and packing.  The
// record semantics are stated at the top of xs_fastx.cpp; oracle/fastx.py is
// the checker (tests/test_fastx.py).  Host code only: no HIP call is made here.
#include "xs_fastx.h"

#include <cstdio>
#include <cstring>

namespace xs::fx {
namespace {

inline bool is_ws(unsigned char c) {
    return c == ' ' || (c >= '\t' && c <= '\r') || (c >= 0x1c && c <= 0x1f);
}

inline const char* rstrip(const char* b, const char* e) {
    while (e > b && is_ws((unsigned char)e[-1])) --e;
    return e;
}

// Next line [b, le) of [p, end) (le excludes '\n'); advances p.
inline bool next_line(const char*& p, const char* end, const char*& b, const char*& le) {
    if (p >= end) return false;
    b = p;
    const char* nl = static_cast<const char*>(memchr(p, '\n', (size_t)(end - p)));
    le = nl ? nl : end;
    p = nl ? nl + 1 : end;
    return true;
}

// Record title (header minus '>'/'@', right-stripped) and id (its first token).
void push_id(Part& out, const char* tb, const char* te) {
    out.descs.append(tb, (size_t)(te - tb));
    out.desc_lens.push_back((uint64_t)(te - tb));
    while (tb < te && is_ws((unsigned char)*tb)) ++tb;
    const char* t = tb;
    while (t < te && !is_ws((unsigned char)*t)) ++t;
    out.ids.append(tb, (size_t)(t - tb));
    out.id_lens.push_back((uint64_t)(t - tb));
}

// FASTA records of [p, end).  `budget`: stop at the first record that starts
// at or beyond p + budget (0: no limit).
void parse_fasta(const char* p, const char* end, size_t budget, Part& out) {
    const char* limit = budget ? p + budget : end;
    const char *b, *le;
    bool have = false;
    size_t seq0 = 0;
    const char* q = p;
    for (;;) {
        const char* line_start = q;
        if (!next_line(q, end, b, le)) break;
        if (le > b && *b == '>') {
            if (have) {
                out.lens.push_back(out.seq.size() - seq0);
                if (line_start >= limit) {
                    out.stop = line_start;
                    return;
                }
            }
            have = true;
            seq0 = out.seq.size();
            push_id(out, b + 1, rstrip(b + 1, le));
        } else if (have) {
            const char* e = rstrip(b, le);
            const char* s = b;
            while (s < e) {  // drop ' ' and '\r' inside the line
                const char* run = s;
                while (s < e && *s != ' ' && *s != '\r') ++s;
                out.seq.append(run, (size_t)(s - run));
                while (s < e && (*s == ' ' || *s == '\r')) ++s;
            }
        }
    }
    if (have) out.lens.push_back(out.seq.size() - seq0);
    out.stop = end;
}

// One FASTQ record as the line rules see it.  Lengths are of right-stripped lines.
struct FqRecord {
    const char* start;          // the header: the first non-blank line
    const char *tb, *te;        // title: the header minus its first character
    size_t seq_lines, slen;     // sequence lines up to the '+' line
    bool plus;                  // a '+' line was found;
    const char *cb, *ce;        // its caption
    size_t qual_lines, qlen;    // quality lines, read until they hold >= slen characters
    const char* stop;           // where the walk ended
};

// Walk one record of [p, end): false if only blank lines are left.  A record
// that starts at or beyond `limit`, or not with '@', is not walked (stop =
// start), and one without a '+' line ends at `end`; the caller tells them
// apart.  `seq`, if not null, receives the sequence lines' characters.
bool walk_fastq(const char* p, const char* end, const char* limit, std::string* seq, FqRecord& r) {
    const char *b, *le;
    do {
        if (!next_line(p, end, b, le)) return false;
    } while (rstrip(b, le) == b);
    r = FqRecord{b, b + 1, rstrip(b + 1, le), 0, 0, false, nullptr, nullptr, 0, 0, b};
    if (b >= limit || *b != '@') return true;
    while (next_line(p, end, b, le)) {
        if (le > b && *b == '+') {
            r.plus = true;
            r.cb = b + 1;
            r.ce = rstrip(b + 1, le);
            break;
        }
        const size_t n = (size_t)(rstrip(b, le) - b);
        if (seq) seq->append(b, n);
        r.slen += n;
        ++r.seq_lines;
    }
    if (r.plus)
        while (r.qlen < r.slen && next_line(p, end, b, le)) {
            r.qlen += (size_t)(rstrip(b, le) - b);
            ++r.qual_lines;
        }
    r.stop = p;
    return true;
}

void fastq_error(Part& out, const char* msg, const FqRecord& r) {
    out.err = std::string(msg) + " (record '" + std::string(r.tb, (size_t)std::min<ptrdiff_t>(r.te - r.tb, 200)) + "')";
}

}  // namespace

void parse_fastq(const char* p, const char* end, size_t budget, Part& out) {
    const char* limit = budget ? p + budget : end;
    FqRecord r;
    for (const char* q = p;; q = r.stop) {
        const size_t seq0 = out.seq.size();
        // the budget holds once a record is held: until then nothing is past it
        if (!walk_fastq(q, end, out.lens.empty() ? end : limit, &out.seq, r)) break;
        if (r.start >= limit && !out.lens.empty()) {
            out.stop = r.start;
            return;
        }
        if (*r.start != '@') {
            out.err = "Records in Fastq files should start with '@' character";
            return;
        }
        if (!r.plus)
            return fastq_error(out, r.slen ? "End of file without quality information." : "Unexpected end of file", r);
        if (r.ce > r.cb && (r.ce - r.cb != r.te - r.tb || memcmp(r.cb, r.tb, (size_t)(r.te - r.tb)) != 0))
            return fastq_error(out, "Sequence and quality captions differ.", r);
        if (memchr(out.seq.data() + seq0, ' ', r.slen) || memchr(out.seq.data() + seq0, '\t', r.slen))
            return fastq_error(out, "Whitespace is not allowed in the sequence.", r);
        if (r.qlen != r.slen) {
            char msg[128];
            snprintf(msg, sizeof(msg), "Lengths of sequence and quality values differs (%zu and %zu).", r.slen, r.qlen);
            return fastq_error(out, msg, r);
        }
        push_id(out, r.tb, r.te);
        out.lens.push_back(r.slen);
    }
    out.stop = end;
}

// Record start at or after `pos` in [lo, end): FASTA '>' at a line start.
const char* fasta_boundary(const char* lo, const char* pos, const char* end) {
    if (pos <= lo) return lo;
    const char* p = pos - 1;
    while (p < end) {
        const char* nl = static_cast<const char*>(memchr(p, '\n', (size_t)(end - p)));
        if (!nl || nl + 1 >= end) return end;
        if (nl[1] == '>') return nl + 1;
        p = nl + 1;
    }
    return end;
}

// FASTQ (4-line records) record start at or after `pos`: a line "@..." whose
// third line starts with '+', whose fourth line is as long as its second, and
// which is followed by end of text or another '@' line.
const char* fastq_boundary(const char* lo, const char* pos, const char* end) {
    if (pos <= lo) return lo;
    const char* p = pos - 1;
    while (p < end) {
        const char* nl = static_cast<const char*>(memchr(p, '\n', (size_t)(end - p)));
        if (!nl || nl + 1 >= end) return end;
        const char* cand = nl + 1;
        p = cand;
        if (*cand != '@') continue;
        const char* q = cand;
        const char *b[4], *le[4];
        int n = 0;
        while (n < 4 && next_line(q, end, b[n], le[n])) ++n;
        if (n < 4) continue;
        if (le[2] <= b[2] || *b[2] != '+') continue;
        if (rstrip(b[1], le[1]) - b[1] != rstrip(b[3], le[3]) - b[3]) continue;
        if (q < end && *q != '@') continue;
        return cand;
    }
    return end;
}

// True if some FASTQ record among the first ones of the file (1 MiB or 1,000
// records) wraps its sequence or quality over several lines; then the file is
// not split.  A malformed record counts as wrapped: the sequential parser
// reports it.  An empty sequence has no quality line to look at.  For any
// other, "one quality line as long as the sequence" is the walk's qual_lines
// == 1 && qlen == slen: the walk reads quality lines until they hold >= slen
// characters, so a first line of slen ends it there; a longer one too, with
// qlen > slen; a shorter one makes it read on, to qual_lines > 1 or to the end
// of the text with qlen < slen; and no line at all leaves qual_lines == 0.
bool fastq_wrapped(const char* p, const char* end) {
    const char* stop = p + std::min<size_t>((size_t)(end - p), 1 << 20);
    FqRecord r;
    for (int records = 0; p < stop && records < 1000; ++records, p = r.stop) {
        if (!walk_fastq(p, end, stop, nullptr, r) || r.start >= stop) break;
        if (*r.start != '@' || !r.plus || r.seq_lines > 1) return true;
        if (r.slen && (r.qual_lines != 1 || r.qlen != r.slen)) return true;
    }
    return false;
}

// Wrapped FASTQ cannot be cut by pattern: the first record start at or after
// `pos`, found by walking the records from the start of the text.  A record
// without '@' or without a '+' line ends the walk there; the part that holds
// a malformed record reports the error when parsed.
const char* fastq_boundary_sequential(const char* lo, const char* pos, const char* end) {
    FqRecord r;
    for (const char* q = lo;; q = r.stop) {
        if (!walk_fastq(q, end, pos, nullptr, r)) return end;
        if (r.start >= pos || *r.start != '@' || !r.plus) return r.start;
    }
}

// Windows ramp up: the reader's k-th window takes at most first_window() << k
// bytes of text (for budgets of at least twice the first), so the caller's
// first probe starts after a small parse while the later, larger windows are
// read behind it.
size_t window_budget(uint64_t max_text_bytes, uint64_t k) {
    const size_t b = std::max<uint64_t>(max_text_bytes, 1);
    const size_t w0 = first_window();
    if (b < 2 * w0 || k >= 16) return b;
    return std::min(b, w0 << k);
}

// End of the window that starts at lo: the first record start at or after
// lo + budget (the whole rest if that is within budget; one record at least).
const char* window_end(const xs_fastx* r, const char* lo, const char* end, size_t budget) {
    auto boundary = r->format == XS_FASTX_FASTA ? fasta_boundary : fastq_boundary;
    const char* hi = (size_t)(end - lo) <= budget ? end : boundary(lo, lo + budget, end);
    if (hi == lo) hi = boundary(lo, lo + 1, end);  // one record larger than the budget
    return hi;
}

// Parse [lo, hi) (cut at record starts) on up to r->threads threads into r->parts.
int parse_window(xs_fastx* r, const char* lo, const char* hi, int* nparts) {
    const bool fasta = r->format == XS_FASTX_FASTA;
    auto boundary = fasta ? fasta_boundary : fastq_boundary;
    const size_t span = (size_t)(hi - lo);
    const int T = (int)std::min<size_t>((size_t)r->threads, std::max<size_t>(1, span >> 20));  // >= 1 MiB per part
    std::vector<const char*> cut(T + 1);
    cut[0] = lo;
    cut[T] = hi;
    for (int i = 1; i < T; ++i) cut[i] = std::max(cut[i - 1], boundary(lo, lo + span * i / T, hi));
    auto work = [&](int i) {
        Part& pt = r->parts[i];
        pt.clear();
        if (cut[i] < cut[i + 1]) {
            if (fasta) parse_fasta(cut[i], cut[i + 1], 0, pt);
            else parse_fastq(cut[i], cut[i + 1], 0, pt);
        } else {
            pt.stop = cut[i + 1];
        }
    };
    xs::parallel_for(T, work);
    r->parts[T - 1].stop = hi;
    *nparts = T;
    for (int i = 0; i < T; ++i)
        if (!r->parts[i].err.empty()) return xs::set_error(XS_ERR_FORMAT, r->parts[i].err.c_str());
    return XS_OK;
}

// Concatenate r->parts[0 .. nparts) into bt (the layout xs_query takes).
int pack_parts(xs_fastx* r, Batch& bt, int nparts) {
    // where each part's records, sequence, id and title bytes begin; the last entries are the totals
    std::vector<uint64_t> rec0(nparts + 1, 0), s0(nparts + 1, 0), i0(nparts + 1, 0), d0(nparts + 1, 0);
    for (int i = 0; i < nparts; ++i) {
        rec0[i + 1] = rec0[i] + r->parts[i].lens.size();
        s0[i + 1] = s0[i] + r->parts[i].seq.size();
        i0[i + 1] = i0[i] + r->parts[i].ids.size();
        d0[i + 1] = d0[i] + r->parts[i].descs.size();
    }
    const uint64_t n = rec0[nparts], sbytes = s0[nparts], ibytes = i0[nparts], dbytes = d0[nparts];
    if (int rc = bt.seqs.ensure(sbytes + 64)) return rc;
    if (int rc = bt.ids.ensure(ibytes + 1)) return rc;
    if (int rc = bt.descs.ensure(dbytes + 1)) return rc;
    for (HostBuf* b : {&bt.offs, &bt.id_offs, &bt.desc_offs})
        if (int rc = b->ensure((n + 1) * 8)) return rc;
    auto* offs = reinterpret_cast<uint64_t*>(bt.offs.p);
    auto* ioffs = reinterpret_cast<uint64_t*>(bt.id_offs.p);
    auto* doffs = reinterpret_cast<uint64_t*>(bt.desc_offs.p);
    auto pack = [&](int i) {
        const Part& pt = r->parts[i];
        if (!pt.seq.empty()) memcpy(bt.seqs.p + s0[i], pt.seq.data(), pt.seq.size());
        if (!pt.ids.empty()) memcpy(bt.ids.p + i0[i], pt.ids.data(), pt.ids.size());
        if (!pt.descs.empty()) memcpy(bt.descs.p + d0[i], pt.descs.data(), pt.descs.size());
        uint64_t so = s0[i], io = i0[i], dd = d0[i];
        for (size_t j = 0; j < pt.lens.size(); ++j) {
            offs[rec0[i] + j] = so;
            ioffs[rec0[i] + j] = io;
            doffs[rec0[i] + j] = dd;
            so += pt.lens[j];
            io += pt.id_lens[j];
            dd += pt.desc_lens[j];
        }
    };
    xs::parallel_for(nparts, pack);
    offs[n] = sbytes;
    ioffs[n] = ibytes;
    doffs[n] = dbytes;
    memset(bt.seqs.p + sbytes, 0, 64);  // defined bytes past the end
    bt.n = n;
    bt.seq_bytes = sbytes;
    return XS_OK;
}

void fill_host_batch(const xs_fastx* r, const Batch& bt, xs_fastx_batch* out) {
    out->n = bt.n;
    out->seqs = bt.seqs.p;
    out->seq_bytes = bt.seq_bytes;
    out->offsets = reinterpret_cast<const uint64_t*>(bt.offs.p);
    out->ids = bt.ids.p;
    out->id_offsets = reinterpret_cast<const uint64_t*>(bt.id_offs.p);
    out->text_offset = r->cur;
    out->text_bytes = r->stop;
    out->descs = bt.descs.p;
    out->desc_offsets = reinterpret_cast<const uint64_t*>(bt.desc_offs.p);
}

}  // namespace xs::fx
