// cls_table_need and cls_table_need_host (include/contivcls.h): the rules a
// table can lose without changing a verdict.  The space, the classes and the
// cells are cls_table_cover's (cover.cpp).  In the reduced form of the rules
// (compile.hpp semantic_rules, family 4, the rules behind one that matches
// every packet kept) "rule k terminates packet x" is a conjunction of three
// tests, so one bit per rule in three row tables gives every cell the set of
// ALL rules that would take it: S[s] & D[d] & C[j] & kept.  Its lowest bit is
// the first match, the next one the rule that takes over when the first is
// deleted.  The device call builds the rows (k_need.hip need_bits), walks the
// cells in tiles of whole (s, d) pairs (need_cells), reduces the tile's arrays
// per rule with cover's fold unchanged (k_cover.hip, as tdiff.cpp does over its
// masked arrays: n_out = R + 2, the sentinel's bin dropped), marks the rules
// (need_mark), runs the cells again for the chained ones when free_out is asked
// for, and fills the witnesses (cover_finish's arithmetic in need_finish).  The
// host call is the same definition in plain C++ over the same rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/contivcls.h"
#include "engine_int.hpp"
#include "kernels.hpp"

static_assert(sizeof(cls_need_witness) == 16, "cls_need_witness is 16 bytes");

namespace {

constexpr uint64_t kNeedMaxCells = 1ull << 40;

size_t even(size_t words) { return (words + 1) & ~size_t(1); }   // a section starts on a whole 16 B

// The sweep's dimensions and the word offsets of the bit rows.
struct NeedDims {
    uint32_t R = 0, W = 1, Ks = 0, Kd = 0, Kt = 0, Ku = 0, T = 0;
    uint64_t pairs = 0, cells = 0;
    size_t wD = 0, wC = 0, wK = 0, words = 0;
    // false: above 2^40 cells
    bool set(uint32_t r, size_t ks, size_t kd, size_t kt, size_t ku) {
        R = r;
        W = std::max<uint32_t>(1, (r + 63) / 64);
        Ks = uint32_t(ks); Kd = uint32_t(kd); Kt = uint32_t(kt); Ku = uint32_t(ku);
        T = Kt + Ku + 2;                                        // <= 2^17 + 2
        pairs = uint64_t(Ks) * Kd;                              // each below 2^32: no overflow
        if (pairs > kNeedMaxCells / T || pairs * T > kNeedMaxCells) return false;
        cells = pairs * T;
        wD = even(size_t(Ks) * W);
        wC = even(wD + size_t(Kd) * W);
        wK = even(wC + size_t(T) * W);
        words = wK + even(W);
        return true;
    }
};

// The kept row: ~skip with the bits from R on clear.
void kept_row(const uint64_t* skip, uint32_t R, uint32_t W, uint64_t* out) {
    for (uint32_t w = 0; w < W; ++w) {
        uint64_t k = skip && w < (R + 63) / 64 ? ~skip[w] : ~0ull;
        const uint64_t lo = uint64_t(w) * 64;
        if (lo + 64 > R) k &= R > lo ? (1ull << (R - lo)) - 1 : 0ull;
        out[w] = k;
    }
}

// The columns as dport | proto << 16 (protocol 3 stands for every value above 2).
void columns(const std::vector<uint16_t>* plo, uint32_t* col) {
    for (uint32_t p = 0; p < 2; ++p)
        for (uint16_t lo : plo[p]) *col++ = uint32_t(lo) | p << 16;
    *col++ = uint32_t(CLS_PROTO_ICMP) << 16;
    *col++ = 3u << 16;
}

bool no_output(const cls_need_out* o) {
    return !o->need_out && !o->free_out && !o->first_out && !o->changed_out && !o->witness_out && !o->counts;
}

// ---- the host form ---------------------------------------------------------
struct HostNeed {
    NeedDims q;
    std::vector<uint64_t> bits;
    std::vector<uint8_t> res;
    // first and second of cell (s, d, j)
    void two(uint32_t s, uint32_t d, uint32_t j, uint32_t& first, uint32_t& second) const {
        const uint64_t *S = &bits[size_t(s) * q.W], *D = &bits[q.wD + size_t(d) * q.W],
                       *C = &bits[q.wC + size_t(j) * q.W], *K = &bits[q.wK];
        first = second = q.R;
        for (uint32_t w = 0; w < q.W; ++w) {
            uint64_t x = S[w] & D[w] & C[w] & K[w];
            while (x) {
                const uint32_t r = 64 * w + uint32_t(__builtin_ctzll(x));
                if (first == q.R) first = r;
                else {
                    second = r;
                    return;
                }
                x &= x - 1;
            }
        }
    }
};

}  // namespace

extern "C" int cls_table_need_host(const cls_rule* rules, uint32_t n_rules, const uint64_t* skip,
                                   const cls_need_out* o) {
    if (!o || no_output(o) || (n_rules && !rules)) return CLS_E_INVAL;
    std::vector<SemRule> sem;
    std::string why;
    if (semantic_rules(rules, n_rules, 4, sem, why, true) != CLS_OK) return CLS_E_INVAL;
    const std::vector<LinRule4> lin = linear4(sem);
    const std::vector<uint32_t> slo = cover_side_starts(rules, n_rules, 0), dlo = cover_side_starts(rules, n_rules, 1);
    const std::vector<uint16_t> plo[2] = {port_class_starts(rules, n_rules, 0), port_class_starts(rules, n_rules, 1)};
    HostNeed H;
    NeedDims& q = H.q;
    if (!q.set(n_rules, slo.size(), dlo.size(), plo[0].size(), plo[1].size())) return CLS_E_INVAL;
    const uint32_t R = q.R;
    std::vector<uint32_t> col(q.T);
    columns(plo, col.data());
    H.bits.assign(q.words, 0);
    H.res.assign(size_t(R) + 1, 0);
    for (const LinRule4& l : lin) {
        const size_t w = l.index >> 6;
        const uint64_t b = 1ull << (l.index & 63);
        H.res[l.index] = need_res_byte(l.meta);
        for (uint32_t s = 0; s < q.Ks; ++s)
            if (need_src_hit(l, slo[s])) H.bits[size_t(s) * q.W + w] |= b;
        for (uint32_t d = 0; d < q.Kd; ++d)
            if (need_dst_hit(l, dlo[d])) H.bits[q.wD + size_t(d) * q.W + w] |= b;
        for (uint32_t j = 0; j < q.T; ++j)
            if (need_col_hit(l, col[j])) H.bits[q.wC + size_t(j) * q.W + w] |= b;
    }
    kept_row(skip, R, q.W, &H.bits[q.wK]);
    std::vector<uint64_t> cnt_first(size_t(R) + 1, 0), cnt_chg(size_t(R) + 1, 0), cnt_chain(size_t(R) + 1, 0),
        min_chg(size_t(R) + 1, ~0ull);
    for (uint32_t s = 0; s < q.Ks; ++s)
        for (uint32_t d = 0; d < q.Kd; ++d)
            for (uint32_t j = 0; j < q.T; ++j) {
                uint32_t f, g;
                H.two(s, d, j, f, g);
                ++cnt_first[f];
                const uint32_t sh = 2 * (col[j] >> 16 & 3);
                if (f < R && (H.res[f] >> sh & 3) != (H.res[g] >> sh & 3)) {
                    ++cnt_chg[f];
                    min_chg[f] = std::min(min_chg[f], (uint64_t(s) * q.Kd + d) * q.T + j);
                }
            }
    std::vector<uint8_t> need(R, 0);
    uint32_t counts[4] = {0, 0, 0, 0};
    for (uint32_t r = 0; r < R; ++r) {
        const bool kept = H.bits[q.wK + (r >> 6)] >> (r & 63) & 1;
        need[r] = !kept ? CLS_NEED_SKIPPED : !cnt_first[r] ? CLS_NEED_DEAD : !cnt_chg[r] ? CLS_NEED_REDUNDANT : CLS_NEED_NEEDED;
        ++counts[need[r]];
    }
    if (o->free_out) {
        for (uint32_t s = 0; s < q.Ks; ++s)
            for (uint32_t d = 0; d < q.Kd; ++d)
                for (uint32_t j = 0; j < q.T; ++j) {
                    uint32_t f, g;
                    H.two(s, d, j, f, g);
                    if (f < R && g < R && need[g] != CLS_NEED_NEEDED) ++cnt_chain[f];
                }
        for (uint32_t r = 0; r < R; ++r)
            o->free_out[r] = need[r] == CLS_NEED_DEAD || (need[r] == CLS_NEED_REDUNDANT && !cnt_chain[r]);
    }
    if (o->need_out && R) std::memcpy(o->need_out, need.data(), R);
    if (o->first_out) std::memcpy(o->first_out, cnt_first.data(), (size_t(R) + 1) * 8);
    if (o->changed_out && R) std::memcpy(o->changed_out, cnt_chg.data(), size_t(R) * 8);
    if (o->counts) std::memcpy(o->counts, counts, sizeof counts);
    if (o->witness_out)
        for (uint32_t r = 0; r < R; ++r) {
            cls_need_witness w{};
            if (need[r] == CLS_NEED_NEEDED) {
                const uint64_t m = min_chg[r], sd = m / q.T;
                const uint32_t j = uint32_t(m - sd * q.T), s = uint32_t(sd / q.Kd), d = uint32_t(sd - uint64_t(s) * q.Kd);
                uint32_t f, g;
                H.two(s, d, j, f, g);
                w.src = slo[s]; w.dst = dlo[d];
                w.dport = uint16_t(col[j]); w.proto = uint8_t(col[j] >> 16);
                w.after = uint8_t(0x80u | (H.res[g] >> (2 * (col[j] >> 16 & 3)) & 3));
                w.fall = g;
            }
            o->witness_out[r] = w;
        }
    if (o->n_cells) *o->n_cells = q.cells;
    if (o->dims) {
        o->dims[0] = q.Ks; o->dims[1] = q.Kd; o->dims[2] = q.Kt; o->dims[3] = q.Ku;
    }
    return CLS_OK;
}

namespace {

// ---- the device form -------------------------------------------------------
// The call's resolved arguments.
struct NeedCall {
    std::shared_ptr<Table> t;
    NeedDims q;
    bool dev = false, cols_lds = false;
    uint64_t tile_pairs = 0;
    size_t off_dlo = 0, off_col = 0, off_res = 0, off_kept = 0, up_bytes = 0;   // in the upload, behind the source starts
    cls_need_out o{};
    hipStream_t s = nullptr;
    size_t rows() const { return size_t(q.R) + 2; }              // the rules, the default, the sentinel
};

// Checks everything a refusal can depend on: no device work is queued, and no
// output written, before this returns CLS_OK.
int need_inputs(cls_engine* e, uint32_t table_id, const cls_need_out* o, uint32_t flags, void* stream, NeedCall& C) {
    const auto it = e->tables.find(table_id);
    if (it == e->tables.end()) return fail(e, CLS_E_NOTFOUND, "no table %u", table_id);
    C.t = it->second;
    if (flags & ~uint32_t(CLS_F_DEVICE)) return fail(e, CLS_E_INVAL, "table need takes CLS_F_DEVICE only");
    if (no_output(o))
        return fail(e, CLS_E_INVAL, "table need without need_out, free_out, first_out, changed_out, witness_out or counts");
    C.dev = flags & CLS_F_DEVICE;
    if (C.dev && (!aligned(o->witness_out, 16) || !aligned(o->first_out, 8) || !aligned(o->changed_out, 8) ||
                  !aligned(o->counts, 4)))
        return fail(e, CLS_E_INVAL, "device table need: witness_out 16-byte, first_out and changed_out 8-byte, counts "
                                    "4-byte aligned");
    NeedDims& q = C.q;
    const Table& t = *C.t;
    if (!q.set(t.n_rules, t.cover_lo[0].size(), t.cover_lo[1].size(), t.port_lo[0].size(), t.port_lo[1].size()))
        return fail(e, CLS_E_INVAL, "table need above 2^40 cells (Ks %u source classes x Kd %u destination classes x T %u "
                                    "columns)", q.Ks, q.Kd, q.T);
    if (q.words * 8 > size_t(e->opts.need_bitmap_mb) << 20)
        return fail(e, CLS_E_INVAL, "table need: bit rows of %zu bytes ((Ks %u + Kd %u + T %u + 1) rows x W %u words) "
                                    "above need_bitmap_mb %u MiB", q.words * 8, q.Ks, q.Kd, q.T, q.W,
                    e->opts.need_bitmap_mb);
    C.tile_pairs = std::max<uint64_t>(1, e->opts.cover_tile / q.T);     // a one-pair tile may exceed cover_tile
    C.cols_lds = e->opts.need_cols_lds && size_t(q.T) * q.W * 8 <= need_cols_lds_max();
    C.s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    C.o = *o;
    C.off_dlo = (size_t(q.Ks) * 4 + 15) & ~size_t(15);
    C.off_col = (C.off_dlo + size_t(q.Kd) * 4 + 15) & ~size_t(15);
    C.off_res = (C.off_col + size_t(q.T) * 4 + 15) & ~size_t(15);
    C.off_kept = (C.off_res + size_t(q.R) + 1 + 15) & ~size_t(15);
    C.up_bytes = C.off_kept + size_t(q.W) * 8;
    return CLS_OK;
}

const std::vector<LinRule4>& need_rules(const Table& t) { return t.need4.empty() ? t.lin4 : t.need4; }

// The class tables, the result bytes and the kept row: one host blob (need_up
// outlives the unsynchronised upload), the first three into v_tab, the kept
// row into the bit rows.
int need_upload(cls_engine* e, const NeedCall& C, const uint64_t* skip) {
    const NeedDims& q = C.q;
    Table& t = *C.t;
    if (!t.need4.empty() && !t.need4_up) {
        HIPC(e, t.d_need4.ensure(t.need4.size() * sizeof(LinRule4)));
        HIPC(e, hipMemcpy(t.d_need4.p, t.need4.data(), t.need4.size() * sizeof(LinRule4), hipMemcpyHostToDevice));
        t.need4_up = true;
    }
    std::vector<uint8_t>& up = e->need_up;
    up.assign(C.up_bytes, 0);
    std::memcpy(up.data(), t.cover_lo[0].data(), size_t(q.Ks) * 4);
    std::memcpy(up.data() + C.off_dlo, t.cover_lo[1].data(), size_t(q.Kd) * 4);
    columns(t.port_lo, reinterpret_cast<uint32_t*>(up.data() + C.off_col));
    for (const LinRule4& l : need_rules(t))
        if (l.index < q.R) up[C.off_res + l.index] = need_res_byte(l.meta);
    kept_row(skip, q.R, q.W, reinterpret_cast<uint64_t*>(up.data() + C.off_kept));
    HIPC(e, e->v_tab.ensure(C.off_kept));
    HIPC(e, e->nd_bits.ensure(q.words * 8));
    HIPC(e, hipMemcpyAsync(e->v_tab.p, up.data(), C.off_kept, hipMemcpyHostToDevice, C.s));
    HIPC(e, hipMemcpyAsync(e->nd_bits.as<uint64_t>() + q.wK, up.data() + C.off_kept, size_t(q.W) * 8,
                           hipMemcpyHostToDevice, C.s));
    return CLS_OK;
}

uint64_t tile_cells(const NeedCall& C) { return std::min(C.tile_pairs, C.q.pairs) * C.q.T; }

// nd_cnt's rows: cells with first == k, changing under k, chained; nd_min's:
// the least changing cell, and one row the other folds write and nobody reads.
unsigned long long* cnt_row(cls_engine* e, const NeedCall& C, int row) {
    return e->nd_cnt.as<unsigned long long>() + size_t(row) * C.rows();
}
unsigned long long* min_row(cls_engine* e, const NeedCall& C, int row) {
    return e->nd_min.as<unsigned long long>() + size_t(row) * C.rows();
}

// A tile's two arrays (the tile rounded up to 1024 cells), the accumulators,
// and whatever output the caller does not take on the device.
int need_scratch(cls_engine* e, const NeedCall& C) {
    const size_t n = size_t((tile_cells(C) + 1023) & ~uint64_t(1023)), r = C.rows(), R = C.q.R;
    HIPC(e, e->v_rule.ensure(n * 4));
    HIPC(e, e->v_mask_a.ensure(n * 4));
    HIPC(e, e->nd_cnt.ensure(3 * r * 8));
    HIPC(e, e->nd_min.ensure(2 * r * 8));
    HIPC(e, hipMemsetAsync(e->nd_cnt.p, 0, 3 * r * 8, C.s));
    HIPC(e, hipMemsetAsync(e->nd_min.p, 0xFF, 2 * r * 8, C.s));
    if (!C.dev || !C.o.need_out) HIPC(e, e->nd_need.ensure(R + 1));      // never null: null selects the first pass
    if (!C.dev && C.o.free_out) HIPC(e, e->nd_free.ensure(R));
    if (!C.dev && C.o.witness_out) HIPC(e, e->nd_wit.ensure(R * 16));
    if (!C.dev && C.o.counts) HIPC(e, e->nd_counts.ensure(16));
    return CLS_OK;
}

NeedTab need_tab(cls_engine* e, const NeedCall& C) {
    const uint8_t* tab = e->v_tab.as<uint8_t>();
    const NeedDims& q = C.q;
    return NeedTab{q.Ks, q.Kd, q.T, q.W, q.R, uint32_t(q.wD), uint32_t(q.wC), uint32_t(q.wK),
                   reinterpret_cast<const uint32_t*>(tab), reinterpret_cast<const uint32_t*>(tab + C.off_dlo),
                   reinterpret_cast<const uint32_t*>(tab + C.off_col), e->nd_bits.as<unsigned long long>(),
                   tab + C.off_res};
}

// One pass over the cells in tiles of whole pairs.  need null: first matches
// and changing cells, folded into rows 0 and 1; else the chained cells, row 2.
int need_pass(cls_engine* e, const NeedCall& C, const NeedTab& q, const uint8_t* need) {
    uint32_t* first = e->v_rule.as<uint32_t>();
    uint32_t* mark = e->v_mask_a.as<uint32_t>();
    const uint32_t n_out = uint32_t(C.rows());
    for (uint64_t p0 = 0; p0 < C.q.pairs; p0 += C.tile_pairs) {
        const uint32_t pairs = uint32_t(std::min(C.tile_pairs, C.q.pairs - p0));
        const uint32_t n = pairs * C.q.T;                      // <= max(2^30, T) cells
        const uint64_t c0 = p0 * C.q.T;
        HIPC(e, launch_need_cells(q, p0, pairs, need, first, mark, C.cols_lds, e->n_cu, C.s));
        if (!need) {
            HIPC(e, launch_cover_fold(c0, n, first, n_out, min_row(e, C, 1), cnt_row(e, C, 0), e->n_cu, C.s));
            HIPC(e, launch_cover_fold(c0, n, mark, n_out, min_row(e, C, 0), cnt_row(e, C, 1), e->n_cu, C.s));
        } else {
            HIPC(e, launch_cover_fold(c0, n, mark, n_out, min_row(e, C, 1), cnt_row(e, C, 2), e->n_cu, C.s));
        }
    }
    return CLS_OK;
}

// Everything behind the upload: the launches into the caller's device memory,
// or into the engine's and from there to the caller's host arrays.  A device
// call is stream-ordered (conn_last).
int need_run(cls_engine* e, const NeedCall& C) {
    const NeedTab q = need_tab(e, C);
    const Table& t = *C.t;
    const size_t R = C.q.R;
    const hipMemcpyKind d2d = hipMemcpyDeviceToDevice, d2h = hipMemcpyDeviceToHost;
    HIPC(e, launch_need_bits(q, t.need4.empty() ? t.d_lin4.as<LinRule4>() : t.d_need4.as<LinRule4>(),
                             uint32_t(need_rules(t).size()), C.s));
    int rc = need_pass(e, C, q, nullptr);
    if (rc != CLS_OK) return rc;
    uint8_t* need = C.dev && C.o.need_out ? C.o.need_out : e->nd_need.as<uint8_t>();
    uint32_t* counts = !C.o.counts ? nullptr : C.dev ? C.o.counts : e->nd_counts.as<uint32_t>();
    unsigned long long* changed = C.dev && C.o.changed_out ? reinterpret_cast<unsigned long long*>(C.o.changed_out)
                                                           : nullptr;
    if (counts) HIPC(e, hipMemsetAsync(counts, 0, 16, C.s));
    HIPC(e, launch_need_mark(q, cnt_row(e, C, 0), cnt_row(e, C, 1), need, counts, changed, C.s));
    uint8_t* free_out = !C.o.free_out ? nullptr : C.dev ? C.o.free_out : e->nd_free.as<uint8_t>();
    if (free_out) {
        rc = need_pass(e, C, q, need);
        if (rc != CLS_OK) return rc;
        HIPC(e, launch_need_free(C.q.R, need, cnt_row(e, C, 2), free_out, C.s));
    }
    uint4* wit = !C.o.witness_out ? nullptr
                 : C.dev          ? reinterpret_cast<uint4*>(C.o.witness_out)
                                  : e->nd_wit.as<uint4>();
    if (wit) HIPC(e, launch_need_finish(q, min_row(e, C, 0), need, wit, C.s));
    if (C.dev) {
        if (C.o.first_out) HIPC(e, hipMemcpyAsync(C.o.first_out, cnt_row(e, C, 0), (R + 1) * 8, d2d, C.s));
        e->conn_last = C.s;
        return CLS_OK;
    }
    if (C.o.need_out && R) HIPC(e, hipMemcpyAsync(C.o.need_out, need, R, d2h, C.s));
    if (free_out && R) HIPC(e, hipMemcpyAsync(C.o.free_out, free_out, R, d2h, C.s));
    if (C.o.first_out) HIPC(e, hipMemcpyAsync(C.o.first_out, cnt_row(e, C, 0), (R + 1) * 8, d2h, C.s));
    if (C.o.changed_out && R) HIPC(e, hipMemcpyAsync(C.o.changed_out, cnt_row(e, C, 1), R * 8, d2h, C.s));
    if (wit && R) HIPC(e, hipMemcpyAsync(C.o.witness_out, wit, R * 16, d2h, C.s));
    if (counts) HIPC(e, hipMemcpyAsync(C.o.counts, counts, 16, d2h, C.s));
    HIPC(e, hipStreamSynchronize(C.s));
    return CLS_OK;
}

}  // namespace

extern "C" int cls_table_need(cls_engine* e, uint32_t table_id, const uint64_t* skip, const cls_need_out* out,
                              uint32_t flags, void* stream) {
    if (!e) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    if (!out) return fail(e, CLS_E_INVAL, "table need without outputs");
    NeedCall C;
    int rc = need_inputs(e, table_id, out, flags, stream, C);
    if (rc != CLS_OK) return rc;
    HIPC(e, hipSetDevice(e->device));
    rc = conn_quiesce(e);        // an earlier stream-ordered call may still use the scratch
    if (rc == CLS_OK) rc = need_upload(e, C, skip);
    if (rc == CLS_OK) rc = need_scratch(e, C);
    if (rc == CLS_OK) rc = need_run(e, C);
    if (rc != CLS_OK) return rc;
    if (out->n_cells) *out->n_cells = C.q.cells;
    if (out->dims) {
        out->dims[0] = C.q.Ks; out->dims[1] = C.q.Kd; out->dims[2] = C.q.Kt; out->dims[3] = C.q.Ku;
    }
    return CLS_OK;
}
