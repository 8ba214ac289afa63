/*
 * xspect_hip.h — C ABI of libxspect_hip.so, the MI355X (gfx950) k-mer x filter
 * probe engine behind the XspecT model classes.
 *
 * The reference crosses a Python<->native FFI once per READ (pybind11 into
 * cobs_index, PyO3 into rbloom with a Python callback per k-mer).  This ABI
 * replaces those crossings with one call per BATCH of reads.  Each entry point
 * names the reference interface it replaces (paths relative to the reference
 * repository):
 *
 *   xs_bank_open            cobs_index.Search(path, True/False)
 *                             src/xspect/models/probabilistic_filter_model.py:389
 *                             src/xspect/models/probabilistic_filter_svm_model.py:313
 *                             src/xspect/models/probabilistic_filter_mlst_model.py:188
 *                           rbloom.Bloom.load(path, hash_func=xxh3_64_intdigest)
 *                             src/xspect/models/probabilistic_single_filter_model.py:155-158
 *   xs_query                Search.search(str(seq), step=step), batched over reads
 *                             probabilistic_filter_model.py:227 (+ _count_kmers :462)
 *                             probabilistic_filter_mlst_model.py:242,274-276
 *                           sum(1 for kmer in _generate_kmers(seq, step) if kmer in bf)
 *                             probabilistic_single_filter_model.py:122-124
 *   xs_query_totals         ModelResult.get_total_hits() + sum(num_kmers)
 *                             src/xspect/models/result.py:57-72,76-90 (device-side)
 *   xs_query_device         same as xs_query on device-resident buffers/stream
 *   xs_bank_create_cobs,    cobs_index.ClassicIndexParameters/classic_construct_list
 *   xs_bank_build,            probabilistic_filter_model.py:186-192
 *   xs_bank_save            CompactIndexParameters/compact_construct_list
 *                             probabilistic_filter_mlst_model.py:132-141
 *   xs_bank_create_bloom    rbloom.Bloom(n, fpr, hash_func), .add(kmer), .save(path)
 *                             probabilistic_single_filter_model.py:88-96
 *
 * Conventions: every int-returning call returns XS_OK (0) or a negative
 * XS_ERR_* code; xs_last_error() returns a thread-local message for the last
 * failure on the calling thread.  No C++ exception leaves the library: a failed
 * host allocation inside a call is XS_ERR_NOMEM, any other C++ runtime failure
 * XS_ERR_INTERNAL (NULL from a pointer-returning call; nothing from a void
 * one).  Host buffers are borrowed for the duration of
 * the call only.  A bank handle owns its device memory and one HIP stream;
 * calls on one handle are serialised by an internal mutex, distinct handles are
 * independent.  The handle's device workspace is shared by all its calls: a
 * call enqueued on a different stream than the handle's previous call (the
 * *_device entry points take the caller's stream) is ordered after that call
 * on the device, so one handle may be used from several streams.  No
 * callbacks into the caller.
 */
#ifndef XSPECT_HIP_H
#define XSPECT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XS_OK 0
#define XS_ERR_ARG (-1)
#define XS_ERR_IO (-2)
#define XS_ERR_FORMAT (-3)
#define XS_ERR_HIP (-4)
#define XS_ERR_UNSUPPORTED (-5)
#define XS_ERR_NOMEM (-6)    /* a host allocation failed inside the call */
#define XS_ERR_INTERNAL (-7) /* any other C++ runtime failure (e.g. a thread could not be started) */

#define XS_BANK_COBS_CLASSIC 0
#define XS_BANK_COBS_COMPACT 1
#define XS_BANK_RBLOOM 2

typedef struct xs_bank xs_bank;

typedef struct xs_bank_info_t {
    int32_t kind;             /* XS_BANK_* */
    int32_t device;           /* HIP device ordinal the bank is resident on */
    uint32_t term_size;       /* k */
    uint32_t num_hashes;      /* COBS h, or rbloom K */
    uint32_t canonicalize;    /* 1: canonical k-mers (always 1 for XspecT banks) */
    uint32_t reserved;
    uint64_t num_docs;        /* D (1 for rbloom) */
    uint64_t num_groups;      /* COBS doc groups (1 for classic) */
    uint64_t page_size;       /* bytes per row per group in the file layout */
    uint64_t signature_rows;  /* sum of signature sizes over groups */
    uint64_t bloom_bits;      /* rbloom bit count (0 for COBS) */
    uint64_t device_bytes;    /* device bytes held by the bank image */
    uint64_t device_row_pitch;/* padded device bytes per row per group */
} xs_bank_info_t;

int xs_version(void);
/* Build id: the first 16 hex digits of a SHA-256 over the library's sources,
 * headers, compiler flags and target, fixed when it was built
 * (xspect2_amd/build.py: source_id).  No reference counterpart: the
 * reference's native dependencies are unpinned (pyproject.toml:16-17), this
 * names exactly which sources a loaded library came from. */
const char* xs_build_id(void);
const char* xs_last_error(void);
int xs_device_count(int* count);

/* Open a bank file and make it resident on `device`.  kind = XS_BANK_*. */
int xs_bank_open(const char* path, int kind, int device, xs_bank** out);
/* A classic COBS index with only docs [doc_lo, doc_hi) resident: each row's
 * byte columns of those docs (doc_lo and doc_hi multiples of 8, or doc_hi the
 * doc count).  One bank column-split over ranks (SURVEY.md §8(e) config 5,
 * option b): every rank hashes every k-mer and reads its slice of each row;
 * the per-read hit columns are then all-gathered (xspect2_amd.distributed). */
int xs_bank_open_docs(const char* path, int device, uint64_t doc_lo, uint64_t doc_hi, xs_bank** out);

/* A bank file's header, read and checked with no device work (no reference
 * counterpart: cobs_index.Search and rbloom.load read the whole file).  *out as
 * xs_bank_info fills it after an open, with device = -1; device_bytes and
 * device_row_pitch are what an open of the whole file allocates, so a caller
 * knows the HBM a model needs before it opens it.  *payload_offset (may be
 * NULL): the file offset of the payload's first byte.
 * Every file refused here is refused by xs_bank_open and xs_bank_open_docs with
 * the same code, before their first HIP call and with *out left NULL;
 * xs_last_error names the path.  XS_ERR_FORMAT: a wrong magic or trailer,
 * version != 1, a header the file's end cuts off, more doc names (or compact
 * groups) than bytes left, per-group num_hashes that differ, zero docs, zero
 * signature or page size, groups that do not cover the docs, a size that does
 * not fit 64 bits (sum(signature sizes) * page size, the compact padding), or
 * a payload that is not exactly the bytes the header implies.
 * XS_ERR_UNSUPPORTED: term_size outside 1..32, num_hashes / rbloom K (compared
 * at their full 64 bits) outside 1..16, canonicalize != 1.
 * One limit is the handle's, not the file's, and is not applied here: the
 * probe's LDS counters hold at most 8192 docs.  xs_bank_open refuses a file of
 * more docs (XS_ERR_UNSUPPORTED, also before any HIP call); xs_bank_open_docs
 * applies the limit to its slice only, so such a bank opens column-split, and
 * this call reports its doc count for the split.
 * xs_bank_create_cobs and xs_bank_create_bloom check their arguments the same
 * way: a size that does not fit 64 bits is XS_ERR_ARG there. */
int xs_bank_file_info(const char* path, int kind, xs_bank_info_t* out, uint64_t* payload_offset);
/* The doc names of a bank file that xs_bank_file_info accepts, each followed by
 * '\n', into buf[cap]; *bytes = the bytes they take.  When *bytes > cap nothing
 * is written: call again with room for *bytes (buf may be NULL with cap 0). */
int xs_bank_file_names(const char* path, int kind, char* buf, uint64_t cap, uint64_t* bytes);

/* Create an empty COBS bank (classic: num_groups = 1 and page_size =
 * ceil(num_docs/8); compact: num_groups groups of 8*page_size docs each, the
 * last one partial).  sig[g] = signature size of group g.  doc_names may be
 * NULL (names "0", "1", ...); a NULL entry is XS_ERR_ARG.  The geometry is
 * checked before sig's entries and the names are read. */
int xs_bank_create_cobs(int device, int kind, uint32_t term_size, uint32_t num_hashes,
                        uint64_t num_docs, uint64_t page_size, uint64_t num_groups,
                        const uint64_t* sig, const char* const* doc_names, xs_bank** out);

/* Create an empty rbloom bank of nbytes bytes and nhash index functions. */
int xs_bank_create_bloom(int device, uint32_t term_size, uint64_t nbytes, uint32_t nhash,
                         xs_bank** out);

/* Insert every k-mer (step 1) of n_rec host records; record r belongs to doc
 * rec_doc[r] (ignored for rbloom; may be NULL there). */
int xs_bank_build(xs_bank* bank, const char* seqs, const uint64_t* offsets,
                  const uint32_t* rec_doc, uint64_t n_rec);
/* Same with device-resident buffers, enqueued on `stream` (NULL = the null stream).
 * A rec_doc entry >= num_docs: xs_bank_build reads the entries on the host and
 * refuses the whole call (XS_ERR_ARG, the image unchanged); here they are in
 * device memory and no entry is read back, so such a record is skipped (none
 * of its k-mers is inserted, no byte outside the image is touched) and every
 * other record of the call is inserted; the call returns XS_OK.  Both calls
 * OR into the image they find: building twice, or over an uploaded image,
 * accumulates. */
int xs_bank_build_device(xs_bank* bank, const void* d_seqs, uint64_t seq_bytes,
                         const uint64_t* d_offsets, const uint32_t* d_rec_doc, uint64_t n_rec,
                         void* stream);

int xs_bank_save(xs_bank* bank, const char* path);
/* Copy the bank back in FILE layout (rows of page_size bytes, groups in order;
 * rbloom: the raw bit bytes). nbytes must equal the file payload size. */
int xs_bank_download(xs_bank* bank, void* host, uint64_t nbytes);
/* Replace the bank image from a FILE-layout payload (the inverse of download).
 * Padding bits, the bits of docs >= num_docs in the last byte of a classic row
 * and in the unused tail of a compact bank's last group, are accepted as they
 * come and ignored: a file of another writer may have them set.  No query
 * reports a doc >= num_docs or lets such a bit into a count, a total or a best
 * doc; download and save give the bytes back unchanged, padding included.  The
 * builders never set a padding bit. */
int xs_bank_upload(xs_bank* bank, const void* host, uint64_t nbytes);

/* rbloom files carry no k-mer length (XspecT keeps it in the model JSON,
 * probabilistic_single_filter_model.py:143-151); set it after xs_bank_open. */
int xs_bank_set_term_size(xs_bank* bank, uint32_t term_size);

int xs_bank_info(const xs_bank* bank, xs_bank_info_t* out);
/* Signature size of each doc group (num_groups entries; COBS banks only). */
int xs_bank_signature_sizes(const xs_bank* bank, uint64_t* out, uint64_t n);
const char* xs_bank_doc_name(const xs_bank* bank, uint64_t i);

/* Probe n reads (host buffers): read r = seqs[offsets[r] .. offsets[r+1]).
 * hits_out: n x D uint32 (row-major, may be NULL), num_kmers_out: n (may be
 * NULL).  k-mers are taken at positions i*step, i < ceil((len-k+1)/step);
 * reads shorter than k contribute no k-mers.
 * Outputs, here and in xs_query_hits, xs_query_totals and xs_query_best: the
 * caller initialises none of them.  A successful call writes every element of
 * every output it is given (n x D hits, n k-mer counts, n best docs and best
 * hits, D or D+1 totals; a read without k-mers gets a row of zeros) and no
 * byte outside them; a call refused because a count may not fit hit_bytes
 * writes nothing.  n = 0 writes the totals only (zeros). */
int xs_query(xs_bank* bank, const char* seqs, const uint64_t* offsets, uint64_t n, uint32_t step,
             uint32_t* hits_out, uint64_t* num_kmers_out);

/* xs_query with the hit matrix in hit_bytes = 1, 2 or 4 bytes per count
 * (uint8 / uint16 / uint32).  A count never exceeds its read's sampled k-mers,
 * so 150 bp reads (130 k-mers) come back in one byte: the matrix is narrowed
 * on the device and a quarter of the bytes cross PCIe.  Fails with XS_ERR_ARG
 * if some read has more k-mers than the width holds. */
int xs_query_hits(xs_bank* bank, const char* seqs, const uint64_t* offsets, uint64_t n, uint32_t step,
                  void* hits_out, int hit_bytes, uint64_t* num_kmers_out);
/* xs_query_hits / xs_query_totals for reads already in HBM (an
 * xs_fastx_dbatch: d_seqs, seq_bytes, d_offsets with [0] = 0, max_len = its
 * longest read, which bounds every count for the width check).  Outputs are
 * host memory, each optional: hits_out n x D (hit_bytes 1, 2 or 4), the
 * sampled k-mer counts, totals_out D+1 (per-doc sums, then the k-mer total).
 * The probe runs in read chunks whose hit rows go back while the next chunk
 * is probed. */
int xs_query_hits_device(xs_bank* bank, const void* d_seqs, uint64_t seq_bytes, const uint64_t* d_offsets,
                         uint64_t n, uint64_t max_len, uint32_t step, void* hits_out, int hit_bytes,
                         uint64_t* num_kmers_out, uint64_t* totals_out);

/* Blocking device -> host copy of `bytes` (e.g. an xs_fastx_dbatch's
 * sequences, for checks). */
int xs_memcpy_to_host(void* host, const void* dev, uint64_t bytes);

/* Device -> device copy of `bytes`, asynchronous on `stream` (e.g. a device
 * reader batch's sequences into a caller's buffer for a collective). */
int xs_memcpy_device(void* dst, const void* src, uint64_t bytes, void* stream);

/* Pinned (page-locked) host memory for outputs the caller reuses across calls:
 * results land there by DMA, with no page faults on a fresh pageable buffer. */
int xs_host_alloc(uint64_t bytes, void** out);
void xs_host_free(void* p);

/* totals_out[d] = sum over reads of hits[r][d] (D entries, uint64),
 * *total_kmers_out = sum of num_kmers.  No per-read matrix is materialised. */
int xs_query_totals(xs_bank* bank, const char* seqs, const uint64_t* offsets, uint64_t n,
                    uint32_t step, uint64_t* totals_out, uint64_t* total_kmers_out);

/* Device-resident variant, asynchronous on `stream` (NULL = the null stream,
 * ordered with all blocking streams; pass torch.cuda.current_stream().cuda_stream).
 * d_seqs holds seq_bytes bytes; d_offsets n+1 uint64.  Any of d_hits (n x D
 * uint32), d_num_kmers (n uint64) and d_totals (D+1 uint64: per-doc totals then
 * the k-mer total) may be NULL.  The bank must live on the current device.
 * No output needs initialising by the caller (the library zeroes the rows it
 * accumulates into, the buffers may hold anything), and nothing outside n x D
 * hits, n k-mer counts and D+1 totals is written; the outputs need 4-byte
 * (hits) and 8-byte alignment only.  n = 0 zeroes d_totals and writes nothing
 * else. */
int xs_query_device(xs_bank* bank, const void* d_seqs, uint64_t seq_bytes,
                    const uint64_t* d_offsets, uint64_t n, uint32_t step, uint32_t* d_hits,
                    uint64_t* d_num_kmers, uint64_t* d_totals, void* stream);

/* Per-read best doc without materialising the hit matrix on the host:
 * best_doc[r] = the doc with the most hits of read r, or XS_BEST_AMBIGUOUS when
 * two or more docs share the maximum (the per-read call of the reference's
 * benchmark, scripts/benchmark/main.nf:417-436); best_hits[r] = that maximum.
 * best_hits, num_kmers_out and totals_out (D+1 entries, as xs_query_totals
 * then the k-mer total) may be NULL. */
#define XS_BEST_AMBIGUOUS 0xFFFFFFFFu
int xs_query_best(xs_bank* bank, const char* seqs, const uint64_t* offsets, uint64_t n, uint32_t step,
                  uint32_t* best_doc, uint32_t* best_hits, uint64_t* num_kmers_out, uint64_t* totals_out);
/* The same reduction over a device hit matrix (n x num_docs uint32) on `stream`. */
int xs_best_device(const uint32_t* d_hits, uint64_t n, uint64_t num_docs, uint32_t* d_best_doc,
                   uint32_t* d_best_hits, void* stream);

/* Device-side read compaction (the genus -> species hand-off of the fused
 * pipeline, replacing the filtered FASTA of src/xspect/main.py:116-145):
 * output read j = input read d_index[j], written at d_out_offsets[j] (m+1
 * entries, computed by the caller from the kept lengths), on `stream`. */
int xs_gather_reads_device(const void* d_seqs, const uint64_t* d_offsets, const uint32_t* d_index, uint64_t m,
                           void* d_out_seqs, const uint64_t* d_out_offsets, void* stream);

/* Read filtering on the device.  The reference decides per read with
 * round(h / n, 2) >= threshold, or for threshold -1 with "the label's rounded
 * score is the read's largest" (ModelResult.get_filter_mask and
 * get_filtered_subsequence_labels, src/xspect/models/result.py:92-149).
 * round(x, 2) is monotone in the double x = h / n, so 101 cuts reproduce it by
 * comparison: cut[c] is the smallest double x with round(x, 2) >= c/100 (ties
 * to even, as Python rounds), and centi(x) = the number of cuts <= x, minus one,
 * is 100 * round(x, 2).  A threshold t in [0, 1] keeps a read iff centi(x) >=
 * min{c : c/100 >= t}; -1 keeps it iff centi(h_label / n) == centi(h_max / n).
 *
 * The 101 cuts (n must be 101), built on the host in exact arithmetic; no
 * device is touched. */
int xs_filter_cuts(double* out, uint64_t n);
/* The keep decision of result.py:92-149 over a device hit matrix (n x num_docs
 * uint32, rows unpadded) and the reads' k-mer counts, on `stream`: d_keep[r] =
 * 1 or 0, d_label_hits[r] (NULL ok) = the label's count.  d_doc_mask (NULL ok):
 * num_docs bytes on the device, a 0 byte drops that doc from the row's maximum
 * (predict's exclude_ids).  The kernel reads it for threshold -1 alone, but a
 * call that passes one, in either mode, first copies the label's byte back and
 * waits for `stream` once, because a masked label is refused; pass NULL with a
 * threshold in [0, 1] to avoid that wait.  A read with no k-mers is never
 * kept.  XS_ERR_ARG: a threshold outside [0, 1] that is not exactly -1 (NaN
 * included), label_doc >= num_docs, a masked label. */
int xs_filter_keep_device(const uint32_t* d_hits, const uint64_t* d_num_kmers, uint64_t n, uint64_t num_docs,
                          uint64_t label_doc, const uint8_t* d_doc_mask, double threshold, uint8_t* d_keep,
                          uint32_t* d_label_hits, void* stream);
/* The kept reads of a batch in file order, replacing the id list and the
 * second parse of file_io.py:166-191 and the hand-off of main.py:116-145:
 * d_index[0..m) = the reads with a non-zero keep byte, ascending; d_out_offsets
 * [0..m] = the running sums of their lengths from 0 (what
 * xs_gather_reads_device takes); d_counts = {m, kept bytes}.  d_offsets: the
 * reads' n + 1 offsets.  A multi-block exclusive scan: deterministic, and
 * nothing past d_index[m - 1], d_out_offsets[m] and d_counts[1] is written.
 * n < 2^32.  The scan's block sums (16 bytes per 1024 reads) are allocated and
 * freed in stream order on the calling thread's current device, which must be
 * the device that owns `stream` and the buffers. */
int xs_filter_compact_device(const uint8_t* d_keep, const uint64_t* d_offsets, uint64_t n, uint32_t* d_index,
                             uint64_t* d_out_offsets, uint64_t* d_counts, void* stream);
/* Probe host reads and keep or drop each (result.py:92-149) without the hit
 * matrix leaving the device: keep_out[r] = 1 or 0.  label_doc: the label's doc
 * index (0 for an rbloom bank); doc_mask: num_docs bytes on the host or NULL;
 * threshold and errors as xs_filter_keep_device.  label_hits_out,
 * num_kmers_out and totals_out (D+1 entries, as xs_query_best) may be NULL.
 * No output needs initialising; every element of every given output is
 * written; n = 0 writes the totals only. */
int xs_query_keep(xs_bank* bank, const char* seqs, const uint64_t* offsets, uint64_t n, uint32_t step,
                  uint64_t label_doc, const uint8_t* doc_mask, double threshold, uint8_t* keep_out,
                  uint32_t* label_hits_out, uint64_t* num_kmers_out, uint64_t* totals_out);

/* MLST chunk scoring (probabilistic_filter_mlst_model.py:237-256): for chunk
 * hit rows hits[c][d] whose owner is seq_of_chunk[c] (non-decreasing), sum
 * hits[c][d] into scores[seq][d] only where hits[c][d] > threshold
 * (get_cobs_result :378).  Host buffers; computed on the device. */
int xs_mlst_sum(xs_bank* bank, const uint32_t* hits, const uint32_t* seq_of_chunk,
                uint64_t n_chunks, uint64_t n_seqs, uint32_t threshold, uint64_t* scores);

/* One MLST locus in one call (probabilistic_filter_mlst_model.py:192-303; the
 * reference makes one cobs search per sequence, and per chunk of every
 * sequence >= 10 kbp, :236-286).  Records [0, n_direct) of seqs/offsets are
 * sequences probed whole: their hit rows come back in direct_hits
 * (n_direct x D uint32).  Records [n_direct, n_direct + n_chunks) are the
 * sequence_splitter chunks (:382-426) of the longer sequences, chunk c owned by
 * sequence chunk_owner[c] (non-decreasing, < n_owners); their rows stay on
 * the device, where per (owner, allele) the chunk scores > threshold
 * (get_cobs_result :377-380) are summed into owner_scores (n_owners x D,
 * :249-252), owner_first gets the first such chunk (index among the chunks,
 * UINT32_MAX if none) and owner_first_score its score: the position at which
 * the reference's all_counts dict first sees the allele, which orders ties of
 * its stable sort by -score (:254-256).  offsets: n_direct + n_chunks + 1
 * entries.  Every output may be NULL (owner_first_score needs owner_first). */
int xs_mlst_query(xs_bank* bank, const char* seqs, const uint64_t* offsets, uint64_t n_direct, uint64_t n_chunks,
                  const uint32_t* chunk_owner, uint64_t n_owners, uint32_t step, uint32_t threshold,
                  uint32_t* direct_hits, uint64_t* owner_scores, uint32_t* owner_first,
                  uint32_t* owner_first_score);

/* ---- MLST typing: the top allele per record and locus, reduced on the device.
 * The reference keeps only the first item of each locus' COBS result per record
 * (probabilistic_filter_mlst_model.py:272-286: score descending, ties by doc
 * index) and the sufficiency test over those scores (:288-303, :428-449).  For
 * a hit row of num_docs counts:
 *   top = the lowest doc holding the row's maximum, top_score = that maximum,
 *   n_tied = the docs holding it (not in the reference: how ambiguous the call is).
 * An all-zero row gives top 0, top_score 0, n_tied num_docs. */
#define XS_MLST_NONE 0xFFFFFFFFu /* no allele (used by the Python layer for "N/A") */

/* The reduction alone, over a device matrix (n x num_docs uint32, row-major),
 * asynchronous on `stream`.  Row r's values are written at index r * out_stride
 * of d_top, d_top_score and d_n_tied (may be NULL), so one call per locus fills
 * one column of n x n_loci arrays (out_stride = n_loci, pointers offset by the
 * locus). */
int xs_mlst_top_device(const uint32_t* d_hits, uint64_t n, uint64_t num_docs, uint32_t* d_top,
                       uint32_t* d_top_score, uint32_t* d_n_tied, uint64_t out_stride, void* stream);

/* Every locus of a scheme for n host reads in one call (replaces the per-locus,
 * per-record index.search loop of probabilistic_filter_mlst_model.py:272-286):
 * the reads are uploaded once, probed against each locus in chunks of R reads
 * (R x the largest locus' docs x 4 bytes <= workspace_bytes, R >= 1; 0: 4 GiB)
 * and each chunk's rows reduced on the device.  No hit matrix crosses to the
 * host.  loci: n_loci distinct COBS banks on one device with one k.  top,
 * top_score, n_tied (NULL ok): n x n_loci, row-major, host memory;
 * num_kmers_out (NULL ok): n entries.  n = 0 writes nothing. */
int xs_mlst_type(xs_bank* const* loci, uint32_t n_loci, const char* seqs, const uint64_t* offsets, uint64_t n,
                 uint32_t step, uint64_t workspace_bytes, uint32_t* top, uint32_t* top_score, uint32_t* n_tied,
                 uint64_t* num_kmers_out);

/* The same for reads already in HBM (an xs_fastx_dbatch: d_seqs, seq_bytes,
 * d_offsets with [0] = 0); outputs are host memory. */
int xs_mlst_type_device(xs_bank* const* loci, uint32_t n_loci, const void* d_seqs, uint64_t seq_bytes,
                        const uint64_t* d_offsets, uint64_t n, uint32_t step, uint64_t workspace_bytes,
                        uint32_t* top, uint32_t* top_score, uint32_t* n_tied, uint64_t* num_kmers_out);

/* ---- MLST typing of contigs: chunk scores and the top allele on the device.
 * The reference treats a record of 10 kbp and more differently
 * (probabilistic_filter_mlst_model.py:236-270): per locus, sequence_splitter
 * (:382-426) cuts it into overlapping chunks of about one allele length, every
 * chunk is searched on its own, only chunk scores > 50 are kept (get_cobs_result
 * :362-380) and summed per allele, and the first allele of the stable sort by
 * -sum is the call (:248-256).  All integers, reproduced exactly:
 *
 *   A record of n >= long_len bytes is long.  With the locus' base width w and
 *   the bank's k: W = w (n < scale10_len), 10 w (n < scale100_len), else 100 w;
 *   stride S = W - k + 1.
 *   n >= W: m = (n - W) / S + 1 full chunks, chunk j = bytes [j S, j S + W).
 *   With r = n - m S (always >= k - 1): r >= k gives one more chunk [m S, n);
 *   r == k - 1 appends the tail to the last chunk, which becomes
 *   seq[(m-1) S : n] + seq[n - (k-1) : n], W + k - 1 bytes with its last k - 1
 *   bytes repeated (the repeat is no window of the record; its junction k-mers
 *   count).  n < W: one chunk, the whole record.
 *   Each chunk is probed as a read with the call's step.  A chunk's count for
 *   an allele takes part only if it is > threshold.  Per (record, allele):
 *   sum of the participating counts, first = the lowest participating chunk,
 *   fscore = that chunk's count.
 *   top = the allele with the largest sum > 0, ties by the lower first, then
 *   the higher fscore, then the lower doc index (the reference's dict order
 *   under its stable sort); top_score = that sum; n_tied = the alleles whose sum
 *   equals it.  No allele with sum > 0: XS_MLST_NONE, 0, 0.
 *
 * Records shorter than long_len follow xs_mlst_type's rule. */
typedef struct xs_mlst_chunk_rule_t {
    uint64_t long_len;      /* records of >= long_len bytes are chunked (reference: 10000, :236) */
    uint64_t scale10_len;   /* from here chunks are 10 x the locus width (1000000, :404-407) */
    uint64_t scale100_len;  /* from here 100 x (10000000, :408-409) */
    uint32_t threshold;     /* a chunk count takes part only if > threshold (50, :378) */
    uint32_t reserved;
} xs_mlst_chunk_rule_t;     /* NULL wherever it is taken: the reference's values */

/* A batch of short reads, contigs or both typed in one call (replaces the loop
 * over loci, chunks and alleles of probabilistic_filter_mlst_model.py:236-286):
 * the reads are uploaded once; short records are probed and reduced as by
 * xs_mlst_type; long records are cut into chunks on the device, the chunks
 * probed, thresholded, summed and reduced there, per locus in ranges of chunks
 * whose rows, texts and accumulators stay within a small multiple of
 * workspace_bytes (0: 4 GiB), a record cut by a range end carrying its sums
 * over.  No text and no per-record matrix returns to the host.  locus_width:
 * n_loci base widths w (the model's average_locus_base_pair_size).  Outputs as
 * xs_mlst_type's; num_kmers_out[r] is the whole record's sampled k-mer count,
 * for long records too.  XS_ERR_ARG beyond xs_mlst_type's: locus_width NULL or
 * some width < k, long_len < k, scale10_len > scale100_len, or 2^32 - 64 and
 * more sequence bytes (a sum could leave uint32). */
int xs_mlst_type_contigs(xs_bank* const* loci, uint32_t n_loci, const uint64_t* locus_width,
                         const xs_mlst_chunk_rule_t* rule, const char* seqs, const uint64_t* offsets, uint64_t n,
                         uint32_t step, uint64_t workspace_bytes, uint32_t* top, uint32_t* top_score,
                         uint32_t* n_tied, uint64_t* num_kmers_out);

/* The same for reads already in HBM.  host_offsets: the n + 1 offsets on the
 * host as well (an xs_fastx_dbatch has them), or NULL: the library copies
 * d_offsets back once, since the lengths decide the chunk geometry. */
int xs_mlst_type_contigs_device(xs_bank* const* loci, uint32_t n_loci, const uint64_t* locus_width,
                                const xs_mlst_chunk_rule_t* rule, const void* d_seqs, uint64_t seq_bytes,
                                const uint64_t* d_offsets, const uint64_t* host_offsets, uint64_t n, uint32_t step,
                                uint64_t workspace_bytes, uint32_t* top, uint32_t* top_score, uint32_t* n_tied,
                                uint64_t* num_kmers_out);

/* The splitter alone (sequence_splitter, probabilistic_filter_mlst_model.py:382-426).
 * xs_mlst_split_size: from the host, the chunks and chunk text bytes that n_long
 * records of the given lengths make at base width `width` (closed forms; every
 * listed record is split, whatever long_len).  xs_mlst_split_device: the chunk
 * texts of records d_long_index[0 .. n_long) of the device reads, repeated
 * tails included, packed into d_chunk_seqs (chunk_bytes + 64 bytes: 64 zero
 * bytes follow the last chunk, as the probes expect), their n_chunks + 1
 * offsets, and per listed record the index of its first chunk (n_long + 1
 * entries, the last = n_chunks).  Returns once they are written.  XS_ERR_ARG:
 * width < k, k = 0, long_len < k, scale10_len > scale100_len. */
int xs_mlst_split_size(const uint64_t* lengths, uint64_t n_long, uint64_t width, uint32_t k,
                       const xs_mlst_chunk_rule_t* rule, uint64_t* n_chunks, uint64_t* chunk_bytes);
int xs_mlst_split_device(const void* d_seqs, const uint64_t* d_offsets, const uint32_t* d_long_index,
                         uint64_t n_long, uint64_t width, uint32_t k, const xs_mlst_chunk_rule_t* rule,
                         void* d_chunk_seqs, uint64_t* d_chunk_offsets, uint64_t* d_owner_begin, void* stream);

/* The reduction alone (probabilistic_filter_mlst_model.py:248-256, 362-380) over
 * a device matrix of chunk rows (n_chunks x num_docs uint32, 4-byte aligned):
 * owner o owns rows [d_owner_begin[o], d_owner_begin[o + 1]) (n_owners + 1
 * non-decreasing entries from 0 to n_chunks; a row's index is its chunk index),
 * an owner without rows gives XS_MLST_NONE, 0, 0.  Owner o's values are written
 * at index o * out_stride of d_top, d_top_score and d_n_tied (may be NULL), as
 * by xs_mlst_top_device.  Returns once they are written. */
int xs_mlst_chunk_top_device(const uint32_t* d_hits, uint64_t n_chunks, uint64_t num_docs,
                             const uint64_t* d_owner_begin, uint64_t n_owners, uint32_t threshold, uint32_t* d_top,
                             uint32_t* d_top_score, uint32_t* d_n_tied, uint64_t out_stride, void* stream);

/* ---- MLST typing: the N best alleles per record and locus, reduced on the device.
 * The reference's `limit` / `limit_number`: the first 5 items of each locus'
 * result under "All results" (probabilistic_filter_mlst_model.py:258-259,
 * 278-282).  N = n_ranks, 1 <= N <= XS_MLST_MAX_RANKS.  All integers:
 *
 *   A record probed whole (a hit row of num_docs counts): the docs ordered by
 *   count descending, then doc index ascending (COBS order); zero counts take
 *   part.  Rank j < min(N, num_docs) is the j-th doc of that order and its
 *   count; ranks j >= num_docs are XS_MLST_NONE, 0.  An all-zero row gives docs
 *   0 .. N-1 with score 0.
 *   A chunked record (xs_mlst_chunk_rule_t): only alleles with sum > 0 take
 *   part, ordered by sum descending, then the lower first passing chunk, then
 *   the higher count in that chunk, then the lower doc (the reference's stable
 *   sort by -sum over its dict, :248-256); ranks beyond their number are
 *   XS_MLST_NONE, 0.
 *
 * Rank 0 is top / top_score of the calls above; n_tied keeps its meaning. */
#define XS_MLST_MAX_RANKS 8

/* The row reduction alone (replaces sorting a whole row to cut its first
 * limit_number items, :278-282), over a device matrix (n x num_docs uint32,
 * row-major, 4-byte aligned), asynchronous on `stream`.  Rank j of row r is
 * written at index r * rank_stride + j of d_rank_allele and d_rank_score
 * (rank_stride >= n_ranks), so one call per locus fills its slice of
 * n x n_loci x n_ranks arrays (rank_stride = n_loci * n_ranks, pointers offset
 * by locus * n_ranks).  d_top, d_top_score and d_n_tied (each may be NULL) get
 * xs_mlst_top_device's values at index r * top_stride, from the same pass. */
int xs_mlst_ranks_device(const uint32_t* d_hits, uint64_t n, uint64_t num_docs, uint32_t n_ranks, uint32_t* d_top,
                         uint32_t* d_top_score, uint32_t* d_n_tied, uint64_t top_stride, uint32_t* d_rank_allele,
                         uint32_t* d_rank_score, uint64_t rank_stride, void* stream);

/* The chunk reduction alone (:248-259) over a device matrix of chunk rows, owners
 * as xs_mlst_chunk_top_device takes them: rank j of owner o at index
 * o * rank_stride + j.  An owner without rows gets XS_MLST_NONE, 0 at every
 * rank.  Returns once they are written. */
int xs_mlst_chunk_ranks_device(const uint32_t* d_hits, uint64_t n_chunks, uint64_t num_docs,
                               const uint64_t* d_owner_begin, uint64_t n_owners, uint32_t threshold, uint32_t n_ranks,
                               uint32_t* d_rank_allele, uint32_t* d_rank_score, uint64_t rank_stride, void* stream);

/* xs_mlst_type_contigs with the ranks (replaces predict(limit=True)'s per-locus
 * searches, whole rows copied back and sorted on the host, :236-286): short
 * records, contigs or both in one call, every argument and output of
 * xs_mlst_type_contigs as there, and rank_allele, rank_score: n x n_loci x
 * n_ranks uint32, row-major, host memory.  The hit rows and the chunk sums are
 * reduced to the ranks on the device; 8 * n_ranks more bytes per (record, locus)
 * go to the host.  XS_ERR_ARG beyond xs_mlst_type_contigs': n_ranks 0 or above
 * XS_MLST_MAX_RANKS, a NULL rank output with n > 0. */
int xs_mlst_type_ranked(xs_bank* const* loci, uint32_t n_loci, const uint64_t* locus_width,
                        const xs_mlst_chunk_rule_t* rule, const char* seqs, const uint64_t* offsets, uint64_t n,
                        uint32_t step, uint64_t workspace_bytes, uint32_t n_ranks, uint32_t* top, uint32_t* top_score,
                        uint32_t* n_tied, uint64_t* num_kmers_out, uint32_t* rank_allele, uint32_t* rank_score);

/* The same for reads already in HBM, as xs_mlst_type_contigs_device takes them. */
int xs_mlst_type_ranked_device(xs_bank* const* loci, uint32_t n_loci, const uint64_t* locus_width,
                               const xs_mlst_chunk_rule_t* rule, const void* d_seqs, uint64_t seq_bytes,
                               const uint64_t* d_offsets, const uint64_t* host_offsets, uint64_t n, uint32_t step,
                               uint64_t workspace_bytes, uint32_t n_ranks, uint32_t* top, uint32_t* top_score,
                               uint32_t* n_tied, uint64_t* num_kmers_out, uint32_t* rank_allele,
                               uint32_t* rank_score);

/* Record HIP events around the probe kernel of every query on this handle. */
int xs_bank_set_profiling(xs_bank* bank, int on);
/* Duration of the probe kernel of the last profiled query, milliseconds. */
int xs_bank_last_probe_ms(xs_bank* bank, float* ms);
/* Count, summed and maximum duration of every probe kernel launched since
 * profiling was enabled or the last call of this function (then resets). */
int xs_bank_probe_stats(xs_bank* bank, uint64_t* count, double* total_ms, float* max_ms);

/* Partitioned probes (xs_bank_probe_path == XS_PATH_PARTITIONED), profiling
 * on: time spent per pass since the last call (then resets), from HIP events
 * on the launch stream at the pass boundaries.  ms[4], count[4] indexed by
 * pass: 0 prep (k-mer counts, scan, block map), 1 bucket (hash, bin by bank
 * partition, transpose), 2 lookup (per-XCD L2-resident partition gathers),
 * 3 resolve (AND per k-mer and count; rbloom: resolve + count).  count =
 * pass instances (one per workspace range). */
int xs_bank_pass_stats(xs_bank* bank, double* ms, uint64_t* count);

/* rbloom banks: filter words the probe kernels loaded since profiling was
 * enabled or the last call (then resets).  The probe tests 2 bits first and
 * loads the other K-2 only for k-mers that pass them, as rbloom stops at the
 * first zero bit, so the count depends on the data; the partitioned path
 * (xs_bank_probe_path) tests all K.  0 for COBS banks, whose kernels read
 * exactly h rows per k-mer and doc group. */
int xs_bank_probe_rows(xs_bank* bank, uint64_t* rows);

/* Probe path of the last query on this handle: XS_PATH_GATHER (one random
 * filter/row gather per hash, every bank kind) or XS_PATH_PARTITIONED (rbloom
 * filters of >= 16 MiB: k-mer bit indices binned by 2 MiB filter partition,
 * each partition tested from one XCD's L2).  The partitioned path is taken
 * while the handle's previous query found at least 24 % of its k-mers in the
 * filter (member-rich input, where it is faster); xs_bank_set_probe_options
 * can disable it.  Both give identical results. */
#define XS_PATH_GATHER 0
#define XS_PATH_PARTITIONED 1
int xs_bank_probe_path(const xs_bank* bank, int* path);

/* Name of the probe kernel the last query on this handle launched, as a
 * NUL-terminated string in buf ("" before the first query; XS_ERR_ARG when cap
 * is too small, 32 bytes hold every name).  The direct COBS probe is one of
 * many compiled instantiations, chosen by the bank's shape: "fast<21,7>"
 * (k, h), "vslice<31,3>" (k or 0, groups), "wide<31,1,C4,G3>" (k, h or 0,0;
 * chunk lanes; groups), "slots<0,0,8,2>" (k, h or 0,0; groups; chunks),
 * "general"; "cobspart" is the partitioned COBS probe; rbloom banks report
 * "bloom<21,7>", "bloom<0,0>" or "bloompart".  The name and the kernel come
 * from one table entry, so tests can hold a bank shape to the kernel it is
 * meant to exercise.  Measurement only: no effect on results. */
int xs_bank_probe_kernel(const xs_bank* bank, char* buf, size_t cap);
/* Every compiled direct COBS probe instantiation, one name per line
 * (XS_ERR_ARG when cap is too small; 4096 bytes hold the list).  Needs no
 * device. */
int xs_probe_kernel_names(char* buf, size_t cap);

/* Probe path selection of one handle.  The defaults (what xs_bank_open and
 * xs_bank_create_* set: 1, 1, 24576, 1) are the paths a production query takes;
 * the other values exist so tests can run every path on the same bank, and no
 * environment variable changes them.  Every path gives identical results.  No
 * reference counterpart (cobs_index / rbloom have one probe each,
 * pyproject.toml:16-17).  Applies to the handle's next query. */
typedef struct xs_probe_options_t {
    int32_t cobs_part;      /* COBS classic banks of <= 128 docs: 0 = direct probe only; 1 = the partitioned
                               probe for banks of >= 32 MiB and calls of >= 2^23 k-mers; 2 = partitioned for
                               every such bank and call; 3 = as 2 with partitions down to 1024 rows; 4 = as 2
                               with partitions of 1024 rows */
    int32_t bloom_part;     /* rbloom: 0 = gather probe only; 1 = partitioned for filters of >= 16 MiB on
                               member-rich input; 2 = such filters whatever the input; 3 = every filter, with
                               partitions down to 1024 bits */
    uint32_t workspace_mib; /* cap of the partitioned COBS probe's transient workspace (a larger call runs in
                               ranges that reuse it) */
    int32_t small_calls;    /* 1: calls of <= 4096 reads and <= 1 MiB go to the device in one round trip;
                               0: every call takes the regular chunked pipeline */
} xs_probe_options_t;
int xs_bank_set_probe_options(xs_bank* bank, const xs_probe_options_t* options);
int xs_bank_get_probe_options(const xs_bank* bank, xs_probe_options_t* options);

/* Device bytes of the handle's transient workspace (staging, reads, hit
 * matrices, the partitioned probes' entries and rows; not the bank image):
 * held now, and the most held at once since the handle was created.  For
 * memory planning beside other work on the GPU (288 GB per MI355X); a doc
 * slice (xs_bank_open_docs) stages one ~32 MiB piece of whole rows at a time,
 * never the whole bank. */
int xs_bank_workspace_bytes(const xs_bank* bank, uint64_t* held, uint64_t* peak);

void xs_bank_close(xs_bank* bank);

/* ---- Result output (src/xspect/models/result.py:151-202, json.dumps(indent=4)).
 * Appends the "hits", "scores" (with "total") and "num_kmers" sections of a
 * ModelResult JSON for an n x num_docs hit matrix to `path`; the caller writes
 * the fields before and after.  hits: counts of hit_bytes = 1, 2 or 4 bytes
 * (uint8/uint16/uint32: a matrix narrowed on the device stays narrow).
 * ids_json / labels_json: packed JSON string literals (quotes included) with
 * n+1 / num_docs+1 offsets; doc_mask (num_docs bytes, 1 = keep) may be NULL.
 * total_hits (num_docs sums), total_kmers and total_order_row (a hit row
 * whose COBS order orders the "total" labels): the whole job's totals for one
 * shard of a read-sharded job (n may then be 0); NULL: computed from this
 * matrix and its first row.  threads <= 0: 16. */
int xs_write_result_sections(const char* path, uint64_t n, uint64_t num_docs, const void* hits, int hit_bytes,
                             const uint64_t* num_kmers, const char* ids_json, const uint64_t* ids_off,
                             const char* labels_json, const uint64_t* labels_off, const uint8_t* doc_mask,
                             const uint64_t* total_hits, uint64_t total_kmers, const uint32_t* total_order_row,
                             int threads);

/* ---- Packed read ids (ASCII only; a byte >= 0x80 is XS_ERR_ARG and the caller
 * falls back to Python).  xs_ids_json_quote: json.dumps(id) of every id (the
 * "hits"/"scores"/"num_kmers" keys ModelResult.save writes, result.py:191-202),
 * packed with n+1 offsets; out_cap >= 6 * offs[n] + 2 * n.
 * xs_ids_has_duplicates: whether two ids are equal (the reference's hits dict
 * keeps the last record of a repeated id, probabilistic_filter_model.py:310). */
int xs_ids_json_quote(const char* buf, const uint64_t* offs, uint64_t n, char* out, uint64_t out_cap,
                      uint64_t* out_offs);
int xs_ids_has_duplicates(const char* buf, const uint64_t* offs, uint64_t n, int* has_dup);
/* out[2i], out[2i+1] = XXH64 of id i with seeds 0 and 0x27D4EB2F165667C5: the
 * 128-bit key by which the ranks of a read-sharded job find ids repeated
 * across their shards (the reference keeps the last record of a repeated id,
 * probabilistic_filter_model.py:310, and sums totals over that dict,
 * result.py:76-90).  Any bytes (not only ASCII). */
int xs_ids_hash128(const char* buf, const uint64_t* offs, uint64_t n, uint64_t* out);
/* out[i] = 1 if keys[i] is one of the m values of `set`, else 0: the owner
 * rank of a read-sharded job finding the records whose key half another
 * record shares (the candidates of a repeated id), in one pass over n keys
 * with a hash set of the (few) shared values.  set may hold repeats. */
int xs_u64_member_mask(const uint64_t* keys, uint64_t n, const uint64_t* set, uint64_t m, uint8_t* out);

/* ---- FASTA/FASTQ reader (host; replaces Bio.SeqIO.parse via
 * get_record_iterator, src/xspect/file_io.py:47-79, on the predict path
 * probabilistic_filter_model.py:316-330).  Records come out packed the way
 * xs_query takes them.  Semantics: see xspect2_amd/csrc/xs_fastx.cpp. */
#define XS_FASTX_FASTA 1
#define XS_FASTX_FASTQ 2
#define XS_FASTX_PINNED 1 /* flag: batch sequence/offset buffers in pinned host memory */

typedef struct xs_fastx xs_fastx;

typedef struct xs_fastx_batch {
    uint64_t n;                  /* records in this batch (0: end of file) */
    uint64_t seq_bytes;          /* bytes of seqs */
    const char* seqs;            /* record r = seqs[offsets[r] .. offsets[r+1]) */
    const uint64_t* offsets;     /* n+1 entries, offsets[0] = 0 */
    const char* ids;             /* record ids (first header token), packed */
    const uint64_t* id_offsets;  /* n+1 entries */
    uint64_t text_offset;        /* file offset parsed up to */
    uint64_t text_bytes;         /* end offset of the reader's text (file size, or its part's end) */
    const char* descs;           /* record titles (header line minus '>'/'@', right-stripped) */
    const uint64_t* desc_offsets;/* n+1 entries */
} xs_fastx_batch;

/* threads <= 0: up to 16.  The file is memory-mapped until xs_fastx_close. */
int xs_fastx_open(const char* path, int format, int threads, int flags, xs_fastx** out);
/* Part `part` of `parts` of the file, for one rank of a read-sharded job
 * (the reference reads the whole file in one
 * process, file_io.py:47-79): the reader yields only the records whose first
 * byte lies in [cut(part), cut(part+1)), cut(i) being the first record start at
 * or after file_size*i/parts.  The parts' records, concatenated in part order,
 * are exactly the file's records.  Each rank maps the file and parses its own
 * slice only.  xs_fastx_open(...) = xs_fastx_open_range(..., 0, 1, ...). */
int xs_fastx_open_range(const char* path, int format, int threads, int flags, uint32_t part, uint32_t parts,
                        xs_fastx** out);
/* Parse the next batch: about max_text_bytes of file text, cut at a record
 * start (one record at least).  Batches ramp up: for budgets of 64 MiB or
 * more, the reader's k-th window takes at most 32 MiB << k, so a pipeline's
 * first probe starts early.  The batch's buffers stay valid until the
 * SECOND following call, so batch i can be probed while batch i+1 is parsed.
 * Malformed records return XS_ERR_FORMAT with Biopython's message. */
int xs_fastx_next(xs_fastx* reader, uint64_t max_text_bytes, xs_fastx_batch* out);
void xs_fastx_close(xs_fastx* reader);

/* Device mode of the same reader (SURVEY.md §8 f1 on the GPU): each window of
 * text — cut exactly as xs_fastx_next cuts it — is copied into pinned memory
 * by host threads and on to HBM, and its records are found on `device`
 * (xs_fastx_dev.hip).  The next window's text is loaded while the caller works
 * on the returned batch.  A window outside the device rules (wrapped FASTQ,
 * blank lines between FASTQ records, empty FASTQ sequences, ' ' or '\r' inside
 * FASTA sequence lines, malformed records) is parsed by the host parser, so
 * batches, ids, titles and error messages equal xs_fastx_next's. */
typedef struct xs_fastx_dbatch {
    uint64_t n;                  /* records in this batch (0: end of the text) */
    uint64_t seq_bytes;          /* bytes of seqs */
    const void* seqs;            /* DEVICE: record r = seqs[offsets[r] .. offsets[r+1]), 64 zero bytes past the end */
    const uint64_t* offsets;     /* DEVICE: n+1 entries, offsets[0] = 0 */
    const uint64_t* host_offsets;/* host: the same n+1 offsets */
    uint64_t max_len;            /* longest record of the batch */
    const char* ids;             /* host: record ids (first header token), packed */
    const uint64_t* id_offsets;  /* host: n+1 entries */
    const char* descs;           /* host: record titles */
    const uint64_t* desc_offsets;/* host: n+1 entries */
    uint64_t text_offset;        /* file offset parsed up to */
    uint64_t text_bytes;         /* end offset of the reader's text */
    int parsed_on_device;        /* 0: this window went through the host parser */
    void* host_ready;            /* the host arrays (host_offsets, ids, descs and their offsets) are
                                    complete once this event has; NULL: already complete.
                                    Wait with xs_fastx_wait_host before reading them */
} xs_fastx_dbatch;

/* As xs_fastx_open_range, for xs_fastx_next_device on `device`. */
int xs_fastx_open_device(const char* path, int format, int threads, int device, uint32_t part, uint32_t parts,
                         xs_fastx** out);
/* Next batch, complete on the device when this returns.  Buffers stay valid
 * until the SECOND following call.  Errors as xs_fastx_next. */
int xs_fastx_next_device(xs_fastx* reader, uint64_t max_text_bytes, xs_fastx_dbatch* out);
/* Block until a device batch's host arrays have landed (their D2H copies run
 * behind the caller's probe of the batch, whose device data is complete when
 * xs_fastx_next_device returns). */
int xs_fastx_wait_host(const xs_fastx_dbatch* batch);

/* Write records as Bio.SeqIO.write(record, fh, "fasta") does (the genus
 * filter's output, src/xspect/file_io.py:166-191): ">" title, then the
 * sequence in lines of `width` (60) characters.  Records r = index[i] for
 * i < n (index NULL: r = i) of a packed batch (seqs/offsets, titles/desc_offs,
 * e.g. an xs_fastx_batch).  append = 0 truncates the file first. */
int xs_write_fasta(const char* path, int append, const char* seqs, const uint64_t* offsets,
                   const char* descs, const uint64_t* desc_offsets, const uint32_t* index, uint64_t n,
                   uint32_t width);

#ifdef __cplusplus
}
#endif
#endif /* XSPECT_HIP_H */
