// xs_bank_header.h — the headers of bank files (COBS classic, COBS compact, rbloom; layouts in xs_bank_io.cpp)
// and the geometry of a bank, read and checked on the host alone.  No HIP header and no xs_bank here: the pair
// xs_bank_header.h / .cpp compiles with any host compiler (tools/asan builds it as it is), and everything it
// refuses is refused before the first HIP call of an open or a create.
//
// Every product and sum that sizes something (G * 8 * page, sum(sig), sum(sig) * page, sum(sig) * pitch, the
// compact padding, an rbloom filter's bits and padded bytes) is computed with overflow checks: a value that does
// not fit 64 bits is XS_ERR_FORMAT from a file and XS_ERR_ARG from arguments.  Reading a header costs work and
// memory in proportion to the file's size whatever its fields claim.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace xs {

// the device's limits (xs_internal.h: kMaxK, kMaxHashes; xs_bank_io.cpp asserts they are the same)
constexpr uint32_t kHeaderMaxK = 32;
constexpr uint32_t kHeaderMaxHashes = 16;
// most doc groups of a compact index (the device's group index is 32 bits; a group takes 16 header bytes)
constexpr uint64_t kHeaderMaxGroups = 1u << 20;

struct BankGeometry {
    int kind = 0;  // XS_BANK_*
    uint32_t k = 0, canonicalize = 1;
    uint64_t h = 0;  // num_hashes / rbloom K at its full width: range-checked before anything narrows it
    uint64_t D = 0, G = 0, page = 0;
    std::vector<uint64_t> sig;
    std::vector<std::string> names;
    uint64_t nbytes = 0;  // rbloom filter bytes
    // derived by check_geometry, all exact
    uint64_t sig_total = 0;      // sum(sig)
    uint64_t payload_bytes = 0;  // sum(sig) * page, or nbytes
    uint64_t pitch = 0;          // COBS: padded device bytes per row
    uint64_t dev_bytes = 0;      // bytes of the device image
    // set by read_bank_header
    uint64_t payload_offset = 0;
};

// Where the geometry came from: decides the code of a value that does not fit 64 bits.
enum class GeometrySource { kFile, kArguments };

// term_size in 1..32 and num_hashes (at its full width) in 1..16, else XS_ERR_UNSUPPORTED with *err set.
int check_term_and_hashes(uint32_t k, uint64_t h, std::string* err);

// The scalar shape of a COBS bank, before its signature sizes and names are touched: docs, groups and page
// size are non-zero and the groups cover the docs exactly ((G - 1) * 8 * page < D <= G * 8 * page).
// XS_OK, or a code with *err set.
int check_cobs_shape(uint64_t D, uint64_t G, uint64_t page, GeometrySource src, std::string* err);

// Checks g (term_size and num_hashes XS_ERR_UNSUPPORTED outside 1..32 / 1..16, then the shape, the signature
// sizes and every size the image and payload need) and fills its derived fields.  XS_OK, or a code with *err set.
int check_geometry(BankGeometry* g, GeometrySource src, std::string* err);

// Reads and checks the header of `path` as a file of `kind`, the payload's size included: on XS_OK g is
// complete and the file holds exactly g->payload_bytes bytes from g->payload_offset.  XS_ERR_IO when the file
// cannot be opened, else XS_ERR_FORMAT / XS_ERR_UNSUPPORTED; *err does not name the path.
int read_bank_header(const char* path, int kind, BankGeometry* g, std::string* err);

}  // namespace xs
