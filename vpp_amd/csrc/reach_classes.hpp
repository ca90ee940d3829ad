// The reachability classes' device-free half (contivcls.h cls_reach_classes,
// cls_reach_classes_host): the keyed mix both the kernels (k_reach_classes.hip)
// and the host fold add up, and the host pipeline -- fold, grouping, verify,
// outputs -- that cls_reach_classes_host runs whole and cls_reach_classes
// (reach.cpp) runs around its two device passes.  No HIP call in here: the
// unit compiles with any C++17 compiler.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/contivcls.h"

#if defined(__HIPCC__)
#define CLS_HD __host__ __device__
#else
#define CLS_HD
#endif

namespace cls {

constexpr uint32_t kClassRounds = 16;     // rounds before "did not converge"
constexpr uint32_t kClassMaxN = 32768;

// splitmix64's finalizer: a bijection of the 64-bit words
CLS_HD inline uint64_t class_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111e5ull;
    x ^= x >> 31;
    return x;
}
// g_row(seed, p, d, value) and g_col(seed, p, s, value): one function, keyed
// by the probe, the position and the byte, under the round's row or column
// seed.  Distinct (p, x, v) give distinct words under one seed.
CLS_HD inline uint64_t class_g(uint64_t seed, uint32_t p, uint32_t x, uint32_t v) {
    return class_mix(seed ^ (uint64_t(p) << 32 | uint64_t(x) << 8 | uint64_t(v)));
}
// the row (which 0) and column (1) seeds of a round: constants, so that a
// result depends on the matrix alone
inline uint64_t class_seed(uint32_t round, uint32_t which) {
    return class_mix(0x9e3779b97f4a7c15ull * (2ull * round + which + 1ull));
}

// One fold pass's results: sums[(p N + s) 2 + {0 row, 1 column}], diag[p N +
// s], mask: bit v set iff byte v occurs in the matrix.
struct ClassFold {
    std::vector<uint64_t> sums;
    std::vector<uint8_t> diag;
    uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
// The fold pass on the host (what reach_class_fold adds up on the device).
void class_fold_host(const uint8_t* m, uint32_t N, uint32_t P, uint32_t round, ClassFold& f);

// Grouping.  Per probe p and byte v present in the matrix, the key of s in a
// round is (row[p][s] + g_row(seed, p, s, v), col[p][s] + g_col(seed, p, s,
// v)) cut to key_bits bits each -- the sums as if the diagonal held v:
// equivalent endpoints whose mutual cells hold v have equal keys under that v
// in every round.  ClassKeys keeps, per (p, v, s), a 64-bit digest of the keys
// of all rounds so far, so a round refines the last ones: endpoints are
// joined (union-find per probe, over all v) when their digests under some v
// and their diagonals agree; the candidate class is the tuple of the probes'
// components.  No endpoint chooses a v: after a collision a choice could
// separate true twins.  Equivalent endpoints are never separated; unequal
// ones stay together only while their keys collide.
struct ClassKeys {
    std::vector<uint8_t> vals;             // the bytes present (the first round's mask)
    std::vector<uint64_t> digest;          // [P][vals][N]
};
// cls receives the candidate, numbered by ascending smallest member; returns C.
uint32_t class_group(uint32_t N, uint32_t P, uint32_t key_bits, uint32_t round, const ClassFold& f, ClassKeys& keys,
                     std::vector<uint32_t>& cls);

// The verify table: [P][C][C + 1] words, entry (p, a, b) the value between
// classes a and b, entry (p, a, C) the diagonal value of a; 0: empty, else
// 0x100 | byte.
constexpr uint32_t kClassEmpty = 0u, kClassSet = 0x100u;
inline size_t class_table_words(uint32_t P, uint32_t C) { return size_t(P) * C * (size_t(C) + 1); }
// The verify pass on the host: fills tab; false on a mismatch.
bool class_verify_host(const uint8_t* m, uint32_t N, uint32_t P, uint32_t C, const uint32_t* cls,
                       std::vector<uint32_t>& tab);

// The per-class outputs of a verified partition and its table.
struct ClassResult {
    std::vector<uint32_t> rep, size;
    std::vector<uint8_t> self, quot;       // [P][C], [P][C][C]
};
void class_result(uint32_t N, uint32_t P, uint32_t C, const uint32_t* cls, const uint32_t* tab, ClassResult& r);

// What both entry points refuse of their outputs and sizes (N, P non-zero and
// within the cell bound are the caller's): null when fine, else the message.
const char* class_refuse(uint32_t N, const cls_reach_classes_out* o);

}  // namespace cls
