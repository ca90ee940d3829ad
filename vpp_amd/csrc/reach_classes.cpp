// The reachability classes on the host (reach_classes.hpp): the fold, the
// grouping, the verify pass, the per-class outputs, and
// cls_reach_classes_host, the device-free twin of cls_reach_classes that runs
// them as one round loop.
#include "reach_classes.hpp"

#include <algorithm>
#include <cstring>
#include <new>
#include <numeric>

namespace cls {

void class_fold_host(const uint8_t* m, uint32_t N, uint32_t P, uint32_t round, ClassFold& f) {
    const uint64_t sr = class_seed(round, 0), sc = class_seed(round, 1);
    f.sums.assign(size_t(P) * N * 2, 0);
    f.diag.assign(size_t(P) * N, 0);
    std::fill(f.mask, f.mask + 8, 0u);
    for (uint32_t p = 0; p < P; ++p) {
        uint64_t* sums = f.sums.data() + size_t(p) * N * 2;
        for (uint32_t s = 0; s < N; ++s) {
            const uint8_t* row = m + (size_t(p) * N + s) * N;
            uint64_t acc = 0;
            for (uint32_t d = 0; d < N; ++d) {
                const uint32_t v = row[d];
                f.mask[v >> 5] |= 1u << (v & 31u);
                if (d == s) continue;
                acc += class_g(sr, p, d, v);
                sums[size_t(d) * 2 + 1] += class_g(sc, p, s, v);
            }
            sums[size_t(s) * 2] = acc;
            f.diag[size_t(p) * N + s] = row[s];
        }
    }
}

namespace {

uint32_t uf_find(std::vector<uint32_t>& up, uint32_t x) {
    while (up[x] != x) {
        up[x] = up[up[x]];
        x = up[x];
    }
    return x;
}

// The first endpoint seen with each key: an open-addressed table of endpoint
// indices (at least twice as many slots as endpoints, so a probe ends).
struct FirstSeen {
    static constexpr uint32_t kNone = ~0u;
    std::vector<uint32_t> slot;
    uint32_t mask = 0;
    explicit FirstSeen(uint32_t n) {
        uint32_t cap = 4;
        while (cap < 2 * n) cap *= 2;
        slot.assign(cap, kNone);
        mask = cap - 1;
    }
    void clear() { std::fill(slot.begin(), slot.end(), kNone); }
    // the endpoint first seen with s's key (s itself when it is the first); same(t, s): equal keys
    template <typename Same> uint32_t first(uint64_t hash, uint32_t s, Same same) {
        for (uint32_t i = uint32_t(class_mix(hash)) & mask;; i = (i + 1) & mask) {
            if (slot[i] == kNone) {
                slot[i] = s;
                return s;
            }
            if (same(slot[i], s)) return slot[i];
        }
    }
};

}  // namespace

uint32_t class_group(uint32_t N, uint32_t P, uint32_t key_bits, uint32_t round, const ClassFold& f, ClassKeys& keys,
                     std::vector<uint32_t>& cls) {
    const uint64_t sr = class_seed(round, 0), sc = class_seed(round, 1);
    const uint64_t keep = key_bits >= 64 ? ~0ull : (1ull << key_bits) - 1ull;
    if (round == 0) {
        keys.vals.clear();
        for (uint32_t v = 0; v < 256; ++v)
            if ((f.mask[v >> 5] >> (v & 31u)) & 1u) keys.vals.push_back(uint8_t(v));
        keys.digest.assign(size_t(P) * keys.vals.size() * N, 0);
    }
    const size_t nv = keys.vals.size();
    std::vector<uint32_t> cur(N, 0), up(N), root(N), id(N);
    FirstSeen seen(N);
    uint32_t C = 1;
    for (uint32_t p = 0; p < P; ++p) {
        const uint64_t* sums = f.sums.data() + size_t(p) * N * 2;
        const uint8_t* diag = f.diag.data() + size_t(p) * N;
        std::iota(up.begin(), up.end(), 0u);
        // the probe's components: endpoints whose digests and diagonals agree under some v
        for (size_t k = 0; k < nv; ++k) {
            const uint32_t v = keys.vals[k];
            uint64_t* dg = keys.digest.data() + (size_t(p) * nv + k) * N;
            seen.clear();
            for (uint32_t s = 0; s < N; ++s) {
                const uint64_t kr = (sums[size_t(s) * 2] + class_g(sr, p, s, v)) & keep;
                const uint64_t kc = (sums[size_t(s) * 2 + 1] + class_g(sc, p, s, v)) & keep;
                dg[s] = class_mix(class_mix(dg[s] ^ kr) + kc);
                const uint32_t t = seen.first(dg[s] + diag[s], s, [&](uint32_t x, uint32_t y) {
                    return dg[x] == dg[y] && diag[x] == diag[y];
                });
                if (t == s) continue;
                const uint32_t a = uf_find(up, t), b = uf_find(up, s);
                if (a != b) up[std::max(a, b)] = std::min(a, b);
            }
        }
        // the candidate so far x this probe's component, numbered by first member
        for (uint32_t s = 0; s < N; ++s) root[s] = uf_find(up, s);
        seen.clear();
        C = 0;
        for (uint32_t s = 0; s < N; ++s) {
            const uint32_t t = seen.first(uint64_t(cur[s]) << 32 | root[s], s, [&](uint32_t x, uint32_t y) {
                return cur[x] == cur[y] && root[x] == root[y];
            });
            id[s] = t == s ? C++ : id[t];
        }
        cur.swap(id);
    }
    cls.swap(cur);
    return C;
}

bool class_verify_host(const uint8_t* m, uint32_t N, uint32_t P, uint32_t C, const uint32_t* cls,
                       std::vector<uint32_t>& tab) {
    tab.assign(class_table_words(P, C), kClassEmpty);
    for (uint32_t p = 0; p < P; ++p)
        for (uint32_t s = 0; s < N; ++s) {
            const uint8_t* row = m + (size_t(p) * N + s) * N;
            uint32_t* t = tab.data() + (size_t(p) * C + cls[s]) * (size_t(C) + 1);
            for (uint32_t d = 0; d < N; ++d) {
                uint32_t& e = t[d == s ? C : cls[d]];
                const uint32_t v = kClassSet | row[d];
                if (e == kClassEmpty) e = v;
                else if (e != v) return false;
            }
        }
    return true;
}

void class_result(uint32_t N, uint32_t P, uint32_t C, const uint32_t* cls, const uint32_t* tab, ClassResult& r) {
    r.rep.assign(C, 0);
    r.size.assign(C, 0);
    for (uint32_t s = N; s-- > 0;) {
        r.rep[cls[s]] = s;
        ++r.size[cls[s]];
    }
    r.self.assign(size_t(P) * C, 0);
    r.quot.assign(size_t(P) * C * C, 0);
    for (size_t pa = 0; pa < size_t(P) * C; ++pa) {
        const uint32_t* t = tab + pa * (size_t(C) + 1);
        r.self[pa] = uint8_t(t[C]);
        // (empty: the intra-class cell of a one-member class)
        for (uint32_t b = 0; b < C; ++b) r.quot[pa * C + b] = t[b] == kClassEmpty ? uint8_t(CLS_CLASS_NONE) : uint8_t(t[b]);
    }
}

const char* class_refuse(uint32_t N, const cls_reach_classes_out* o) {
    if (!o) return "reach classes without outputs";
    if (!o->class_out && !o->n_classes) return "reach classes without class_out or n_classes";
    if (N > kClassMaxN) return "reach classes above 32768 endpoints";
    if ((o->rep_out || o->size_out || o->self_out || o->quot_out) && !o->class_cap)
        return "reach classes: per-class outputs with class_cap 0";
    return nullptr;
}

}  // namespace cls

using namespace cls;

extern "C" int cls_reach_classes_host(const uint8_t* matrix, uint32_t N, uint32_t P, uint32_t key_bits,
                                      const cls_reach_classes_out* o) {
    if (!matrix || !N || !P || key_bits > 64 || class_refuse(N, o)) return CLS_E_INVAL;
    if (uint64_t(N) * N > (1ull << 36) / P) return CLS_E_INVAL;
    try {
        std::vector<uint32_t> cand, tab;
        ClassFold f;
        ClassKeys keys;
        uint32_t C = 0, round = 0;
        bool ok = false;
        for (; round < kClassRounds && !ok; ++round) {
            class_fold_host(matrix, N, P, round, f);
            C = class_group(N, P, key_bits, round, f, keys, cand);
            ok = class_verify_host(matrix, N, P, C, cand.data(), tab);
        }
        if (!ok) return CLS_E_INVAL;               // did not converge (key_bits)
        if (o->rounds) *o->rounds = round;
        if (o->sums_out) std::memcpy(o->sums_out, f.sums.data(), f.sums.size() * 8);
        if (o->verdict_out && o->verdict_out != matrix) std::memcpy(o->verdict_out, matrix, size_t(P) * N * N);
        if (o->class_out) std::memcpy(o->class_out, cand.data(), size_t(N) * 4);
        if (o->n_classes) *o->n_classes = C;
        if (C > o->class_cap) return CLS_OK;
        ClassResult r;
        class_result(N, P, C, cand.data(), tab.data(), r);
        if (o->rep_out) std::memcpy(o->rep_out, r.rep.data(), size_t(C) * 4);
        if (o->size_out) std::memcpy(o->size_out, r.size.data(), size_t(C) * 4);
        if (o->self_out) std::memcpy(o->self_out, r.self.data(), r.self.size());
        if (o->quot_out) std::memcpy(o->quot_out, r.quot.data(), r.quot.size());
        return CLS_OK;
    } catch (const std::bad_alloc&) {
        return CLS_E_NOMEM;
    }
}
