// cls_table_diff (include/contivcls.h): the packets whose verdict differs
// between two tables.  Both tables' verdicts are constant on every cell of the
// joint classes (cover.cpp: evalACL sees a packet through Contains tests per
// side, one protocol switch and port-range comparisons; the joint classes are
// those of the two rule lists concatenated, the sorted union of the tables'
// class starts).  The Ks Kd rows of T cells go through in tiles of whole rows:
// per tile one expand launch over the joint class tables (k_cover.hip),
// classify_rules_locked unchanged once per table (verdicts and terminating
// rules), the compare launch (k_tdiff.hip), cover's fold over each masked rule
// array, and for the records the scan and the emit launch; cover's finish
// launch at the end for the witnesses.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <iterator>
#include <mutex>
#include <vector>

#include "../../include/contivcls.h"
#include "engine_int.hpp"
#include "kernels.hpp"

static_assert(sizeof(cls_tdiff_rec) == 32, "cls_tdiff_rec is 32 bytes");

namespace {

constexpr uint64_t kDiffMaxCells = 1ull << 40;
// the call's u64 words in v_dacc: the 16 pair bins, n_diff, the record total, the least differing cell
constexpr size_t kAccPairs = 0, kAccDiff = 16, kAccRec = 17, kAccFirst = 18, kAccWords = 19;

template <typename T>
std::vector<T> joint(const std::vector<T>& a, const std::vector<T>& b) {
    std::vector<T> v;
    std::set_union(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(v));
    return v;
}

// The call's resolved arguments.
struct DiffCall {
    std::shared_ptr<Table> ta, tb;
    uint32_t id_a = 0, id_b = 0;
    bool k16 = false, linear = false, dev = false, recs = false;
    std::vector<uint32_t> slo, dlo;
    std::vector<uint16_t> plo[2];
    uint32_t Ks = 0, Kd = 0, Kt = 0, Ku = 0, T = 0;
    uint64_t rows = 0, cells = 0, tile_rows = 0;
    size_t off_dlo = 0, off_col = 0, tab_bytes = 0;   // in the class tables' blob, behind the source starts
    cls_tdiff_out o{};
    hipStream_t s = nullptr;
    uint32_t ra() const { return ta->n_rules; }
    uint32_t rb() const { return tb->n_rules; }
};

// Checks everything a refusal can depend on: no device work is queued, and no
// output written, before this returns CLS_OK.
int diff_inputs(cls_engine* e, uint32_t table_a, uint32_t table_b, uint32_t af, const cls_tdiff_out* o, uint32_t flags,
                void* stream, DiffCall& C) {
    const auto ia = e->tables.find(table_a), ib = e->tables.find(table_b);
    if (ia == e->tables.end()) return fail(e, CLS_E_NOTFOUND, "no table %u", table_a);
    if (ib == e->tables.end()) return fail(e, CLS_E_NOTFOUND, "no table %u", table_b);
    C.ta = ia->second;
    C.tb = ib->second;
    C.id_a = table_a;
    C.id_b = table_b;
    if (af != CLS_AF_V4 && af != CLS_AF_V16) return fail(e, CLS_E_INVAL, "af must be CLS_AF_V4 or CLS_AF_V16");
    if (af == CLS_AF_V16 && !C.ta->p16.ok)
        return fail(e, CLS_E_INVAL, "no 16-byte classifier for this table (%u): %s", table_a, C.ta->p16.why.c_str());
    if (af == CLS_AF_V16 && !C.tb->p16.ok)
        return fail(e, CLS_E_INVAL, "no 16-byte classifier for this table (%u): %s", table_b, C.tb->p16.why.c_str());
    if (flags & ~uint32_t(CLS_F_DEVICE | CLS_F_FORCE_LINEAR))
        return fail(e, CLS_E_INVAL, "table diff takes CLS_F_DEVICE and CLS_F_FORCE_LINEAR only");
    if (!o->n_diff && !o->pairs_out && !o->first_out && !o->cells_a && !o->wit_a && !o->cells_b && !o->wit_b &&
        !o->rec_out && !o->n_rec)
        return fail(e, CLS_E_INVAL, "table diff without any output");
    if (o->rec_out && !o->n_rec) return fail(e, CLS_E_INVAL, "table diff: rec_out without n_rec");
    if (o->rec_cap && !o->rec_out) return fail(e, CLS_E_INVAL, "table diff: rec_cap %llu without rec_out",
                                               (unsigned long long)o->rec_cap);
    C.dev = flags & CLS_F_DEVICE;
    if (C.dev && (!aligned(o->rec_out, 16) || !aligned(o->first_out, 16) || !aligned(o->wit_a, 16) ||
                  !aligned(o->wit_b, 16) || !aligned(o->n_diff, 8) || !aligned(o->pairs_out, 8) ||
                  !aligned(o->cells_a, 8) || !aligned(o->cells_b, 8) || !aligned(o->n_rec, 8)))
        return fail(e, CLS_E_INVAL, "device table diff: records and witnesses 16-byte, u64 arrays 8-byte aligned");
    C.linear = flags & CLS_F_FORCE_LINEAR;
    C.k16 = af == CLS_AF_V16 && !C.linear;                  // the linear kernel is the IPv4 one (cover.cpp)
    C.slo = joint(C.ta->cover_lo[0], C.tb->cover_lo[0]);
    C.dlo = joint(C.ta->cover_lo[1], C.tb->cover_lo[1]);
    for (int p = 0; p < 2; ++p) C.plo[p] = joint(C.ta->port_lo[p], C.tb->port_lo[p]);
    C.Ks = uint32_t(C.slo.size());
    C.Kd = uint32_t(C.dlo.size());
    C.Kt = uint32_t(C.plo[0].size());
    C.Ku = uint32_t(C.plo[1].size());
    C.T = C.Kt + C.Ku + 2;                                  // <= 2^17 + 2
    C.rows = uint64_t(C.Ks) * C.Kd;                         // each below 2^32: no overflow
    if (C.rows > kDiffMaxCells / C.T || C.rows * C.T > kDiffMaxCells)
        return fail(e, CLS_E_INVAL, "table diff above 2^40 cells (Ks %u source classes x Kd %u destination classes x "
                                    "T %u columns)", C.Ks, C.Kd, C.T);
    C.cells = C.rows * C.T;
    C.tile_rows = std::max<uint64_t>(1, e->opts.cover_tile / C.T);   // a one-row tile may exceed cover_tile
    C.recs = o->n_rec != nullptr;
    C.s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    C.o = *o;
    C.off_dlo = (size_t(C.Ks) * 4 + 15) & ~size_t(15);
    C.off_col = (C.off_dlo + size_t(C.Kd) * 4 + 15) & ~size_t(15);
    C.tab_bytes = C.off_col + ((size_t(C.T) * 4 + 15) & ~size_t(15));
    return CLS_OK;
}

// The joint class tables in cover's blob: source starts, destination starts,
// the columns (dport | proto << 16; protocol 3 stands for every value above 2).
int diff_upload(cls_engine* e, const DiffCall& C) {
    std::vector<uint8_t>& up = e->cover_up;                  // outlives the unsynchronised upload
    up.assign(C.tab_bytes, 0);
    std::memcpy(up.data(), C.slo.data(), size_t(C.Ks) * 4);
    std::memcpy(up.data() + C.off_dlo, C.dlo.data(), size_t(C.Kd) * 4);
    uint32_t* col = reinterpret_cast<uint32_t*>(up.data() + C.off_col);
    for (uint32_t p = 0; p < 2; ++p)
        for (uint16_t lo : C.plo[p]) *col++ = uint32_t(lo) | p << 16;
    *col++ = uint32_t(CLS_PROTO_ICMP) << 16;
    *col++ = 3u << 16;
    HIPC(e, e->v_tab.ensure(C.tab_bytes));
    HIPC(e, hipMemcpyAsync(e->v_tab.p, up.data(), C.tab_bytes, hipMemcpyHostToDevice, C.s));
    return CLS_OK;
}

uint64_t tile_cells(const DiffCall& C) { return std::min(C.tile_rows, C.rows) * C.T; }

// The call's u64 words: the caller's with CLS_F_DEVICE where given, else the engine's.
unsigned long long* acc_word(cls_engine* e, const DiffCall& C, uint64_t* given, size_t at) {
    return C.dev && given ? reinterpret_cast<unsigned long long*>(given) : e->v_dacc.as<unsigned long long>() + at;
}

// A tile's arrays (whole groups of four cells: the tile rounded up to 1024),
// the accumulators, and whatever output the caller does not take on the device.
int diff_scratch(cls_engine* e, const DiffCall& C) {
    const size_t n = size_t((tile_cells(C) + 1023) & ~uint64_t(1023));
    const size_t ra = size_t(C.ra()) + 2, rb = size_t(C.rb()) + 2;      // the rules, the default, the sentinel
    HIPC(e, e->v_src.ensure(n * (C.k16 ? 16 : 4)));
    HIPC(e, e->v_dst.ensure(n * (C.k16 ? 16 : 4)));
    HIPC(e, e->v_dport.ensure(n * 2));
    HIPC(e, e->v_proto.ensure(n));
    HIPC(e, e->v_was.ensure(n));
    HIPC(e, e->v_now.ensure(n));
    HIPC(e, e->v_rule.ensure(n * 4));
    HIPC(e, e->v_rule_b.ensure(n * 4));
    HIPC(e, e->v_mask_a.ensure(n * 4));
    HIPC(e, e->v_mask_b.ensure(n * 4));
    HIPC(e, e->v_min.ensure(ra * 8));
    HIPC(e, e->v_min_b.ensure(rb * 8));
    HIPC(e, e->v_cnt.ensure(ra * 8));
    HIPC(e, e->v_cnt_b.ensure(rb * 8));
    HIPC(e, e->v_dacc.ensure(kAccWords * 8));
    HIPC(e, hipMemsetAsync(e->v_min.p, 0xFF, ra * 8, C.s));
    HIPC(e, hipMemsetAsync(e->v_min_b.p, 0xFF, rb * 8, C.s));
    HIPC(e, hipMemsetAsync(e->v_cnt.p, 0, ra * 8, C.s));
    HIPC(e, hipMemsetAsync(e->v_cnt_b.p, 0, rb * 8, C.s));
    HIPC(e, hipMemsetAsync(e->v_dacc.p, 0, kAccFirst * 8, C.s));
    HIPC(e, hipMemsetAsync(e->v_dacc.as<unsigned long long>() + kAccFirst, 0xFF, 8, C.s));
    if (C.dev && C.o.pairs_out) HIPC(e, hipMemsetAsync(C.o.pairs_out, 0, 16 * 8, C.s));
    if (C.dev && C.o.n_diff) HIPC(e, hipMemsetAsync(C.o.n_diff, 0, 8, C.s));
    if (C.dev && C.o.n_rec) HIPC(e, hipMemsetAsync(C.o.n_rec, 0, 8, C.s));
    if (C.recs) {
        const size_t chunks = (n + kReachChunk - 1) / kReachChunk;
        HIPC(e, e->v_dcount.ensure(chunks * 4));
        HIPC(e, e->v_dbase.ensure(chunks * 8));
    }
    if (!C.dev) {
        if (C.o.wit_a) HIPC(e, e->v_wit.ensure((ra - 1) * 16));
        if (C.o.wit_b) HIPC(e, e->v_wit_b.ensure((rb - 1) * 16));
        if (C.o.first_out) HIPC(e, e->v_first.ensure(16));
        // no more runs than cells
        if (C.o.rec_out && C.o.rec_cap) HIPC(e, e->v_rec.ensure(size_t(std::min<uint64_t>(C.o.rec_cap, C.cells)) * 32));
    }
    return CLS_OK;
}

CoverTile tile_of(cls_engine* e, const DiffCall& C, uint64_t c0, uint32_t n) {
    const uint8_t* tab = e->v_tab.as<uint8_t>();
    return CoverTile{c0, n, C.Kd, C.T, reinterpret_cast<const uint32_t*>(tab),
                     reinterpret_cast<const uint32_t*>(tab + C.off_dlo),
                     reinterpret_cast<const uint32_t*>(tab + C.off_col)};
}

uint4* diff_rec(cls_engine* e, const DiffCall& C) {
    return !C.o.rec_out || !C.o.rec_cap ? nullptr
           : C.dev                      ? reinterpret_cast<uint4*>(C.o.rec_out)
                                        : e->v_rec.as<uint4>();
}

// One tile: the n cells (whole rows) from c0 on.
int diff_tile(cls_engine* e, const DiffCall& C, uint64_t c0, uint32_t n) {
    const CoverTile t = tile_of(e, C, c0, n);
    HIPC(e, launch_cover_expand(t, C.k16, e->v_src.p, e->v_dst.p, e->v_dport.as<uint16_t>(), e->v_proto.as<uint8_t>(),
                                e->n_cu, C.s));
    // the evaluator, unchanged: the matched-rule trace of a device batch, once per table
    cls_pkt_soa pk{};
    pk.af = C.k16 ? CLS_AF_V16 : CLS_AF_V4;
    if (C.k16) {
        pk.src16 = e->v_src.as<uint8_t>(); pk.dst16 = e->v_dst.as<uint8_t>();
    } else {
        pk.src4 = e->v_src.as<uint32_t>(); pk.dst4 = e->v_dst.as<uint32_t>();
    }
    pk.dport = e->v_dport.as<uint16_t>();
    pk.proto = e->v_proto.as<uint8_t>();
    int rc = classify_rules_locked(e, C.id_a, &pk, n, e->v_was.as<uint8_t>(), e->v_rule.as<uint32_t>(), CLS_F_DEVICE,
                                   C.s, C.linear);
    if (rc == CLS_OK)
        rc = classify_rules_locked(e, C.id_b, &pk, n, e->v_now.as<uint8_t>(), e->v_rule_b.as<uint32_t>(), CLS_F_DEVICE,
                                   C.s, C.linear);
    if (rc != CLS_OK) return rc;
    const TDiffTile q{t, C.Ks, C.Kt, C.Ku};
    const TDiffCells cells{e->v_was.as<uint8_t>(), e->v_now.as<uint8_t>(), e->v_rule.as<uint32_t>(),
                           e->v_rule_b.as<uint32_t>()};
    unsigned long long* acc = e->v_dacc.as<unsigned long long>();
    uint32_t* count = C.recs ? e->v_dcount.as<uint32_t>() : nullptr;
    HIPC(e, launch_tdiff_count(q, cells, C.ra() + 1, C.rb() + 1, e->v_mask_a.as<uint32_t>(),
                               e->v_mask_b.as<uint32_t>(), count, acc_word(e, C, C.o.pairs_out, kAccPairs),
                               acc_word(e, C, C.o.n_diff, kAccDiff), acc + kAccFirst, e->n_cu, C.s));
    // per rule: the least differing cell and the differing cells; the sentinel's bin is dropped
    if (C.o.cells_a || C.o.wit_a)
        HIPC(e, launch_cover_fold(c0, n, e->v_mask_a.as<uint32_t>(), C.ra() + 2, e->v_min.as<unsigned long long>(),
                                  e->v_cnt.as<unsigned long long>(), e->n_cu, C.s));
    if (C.o.cells_b || C.o.wit_b)
        HIPC(e, launch_cover_fold(c0, n, e->v_mask_b.as<uint32_t>(), C.rb() + 2, e->v_min_b.as<unsigned long long>(),
                                  e->v_cnt_b.as<unsigned long long>(), e->n_cu, C.s));
    if (C.recs) {
        HIPC(e, launch_reach_diff_scan(uint32_t((uint64_t(n) + kReachChunk - 1) / kReachChunk), count,
                                       e->v_dbase.as<unsigned long long>(), acc_word(e, C, C.o.n_rec, kAccRec), C.s));
        HIPC(e, launch_tdiff_emit(q, cells, count, e->v_dbase.as<unsigned long long>(), diff_rec(e, C), C.o.rec_cap,
                                  e->n_cu, C.s));
    }
    return CLS_OK;
}

// The finish launches into the caller's device memory, or into the engine's
// and from there to the caller's host arrays.  A device call is stream-ordered
// (conn_last).
int diff_outputs(cls_engine* e, const DiffCall& C) {
    const uint32_t ra = C.ra() + 1, rb = C.rb() + 1;
    const CoverTile t = tile_of(e, C, 0, 0);
    unsigned long long* acc = e->v_dacc.as<unsigned long long>();
    uint4* wa = !C.o.wit_a ? nullptr : C.dev ? reinterpret_cast<uint4*>(C.o.wit_a) : e->v_wit.as<uint4>();
    uint4* wb = !C.o.wit_b ? nullptr : C.dev ? reinterpret_cast<uint4*>(C.o.wit_b) : e->v_wit_b.as<uint4>();
    uint4* wf = !C.o.first_out ? nullptr : C.dev ? reinterpret_cast<uint4*>(C.o.first_out) : e->v_first.as<uint4>();
    if (wa) HIPC(e, launch_cover_finish(t, e->v_min.as<unsigned long long>(), ra, nullptr, wa, nullptr, C.s));
    if (wb) HIPC(e, launch_cover_finish(t, e->v_min_b.as<unsigned long long>(), rb, nullptr, wb, nullptr, C.s));
    if (wf) HIPC(e, launch_cover_finish(t, acc + kAccFirst, 1, nullptr, wf, nullptr, C.s));
    if (C.dev) {
        const hipMemcpyKind kind = hipMemcpyDeviceToDevice;
        if (C.o.cells_a) HIPC(e, hipMemcpyAsync(C.o.cells_a, e->v_cnt.p, size_t(ra) * 8, kind, C.s));
        if (C.o.cells_b) HIPC(e, hipMemcpyAsync(C.o.cells_b, e->v_cnt_b.p, size_t(rb) * 8, kind, C.s));
        e->conn_last = C.s;
        return CLS_OK;
    }
    const hipMemcpyKind kind = hipMemcpyDeviceToHost;
    uint64_t words[kAccWords];
    HIPC(e, hipMemcpyAsync(words, acc, sizeof words, kind, C.s));
    if (wa) HIPC(e, hipMemcpyAsync(C.o.wit_a, wa, size_t(ra) * 16, kind, C.s));
    if (wb) HIPC(e, hipMemcpyAsync(C.o.wit_b, wb, size_t(rb) * 16, kind, C.s));
    if (wf) HIPC(e, hipMemcpyAsync(C.o.first_out, wf, 16, kind, C.s));
    if (C.o.cells_a) HIPC(e, hipMemcpyAsync(C.o.cells_a, e->v_cnt.p, size_t(ra) * 8, kind, C.s));
    if (C.o.cells_b) HIPC(e, hipMemcpyAsync(C.o.cells_b, e->v_cnt_b.p, size_t(rb) * 8, kind, C.s));
    HIPC(e, hipStreamSynchronize(C.s));
    if (C.o.pairs_out) std::memcpy(C.o.pairs_out, words + kAccPairs, 16 * 8);
    if (C.o.n_diff) *C.o.n_diff = words[kAccDiff];
    if (C.o.n_rec) *C.o.n_rec = words[kAccRec];
    if (const uint64_t got = std::min<uint64_t>(words[kAccRec], C.o.rec_cap); got && diff_rec(e, C)) {
        HIPC(e, hipMemcpyAsync(C.o.rec_out, e->v_rec.p, size_t(got) * 32, kind, C.s));
        HIPC(e, hipStreamSynchronize(C.s));
    }
    return CLS_OK;
}

}  // namespace

extern "C" int cls_table_diff(cls_engine* e, uint32_t table_a, uint32_t table_b, uint32_t af, const cls_tdiff_out* out,
                              uint32_t flags, void* stream) {
    if (!e) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    if (!out) return fail(e, CLS_E_INVAL, "table diff without outputs");
    DiffCall C;
    int rc = diff_inputs(e, table_a, table_b, af, out, flags, stream, C);
    if (rc != CLS_OK) return rc;
    HIPC(e, hipSetDevice(e->device));
    rc = conn_quiesce(e);        // an earlier stream-ordered call may still use the scratch
    if (rc == CLS_OK) rc = diff_upload(e, C);
    if (rc == CLS_OK) rc = diff_scratch(e, C);
    const uint64_t tile = tile_cells(C);
    for (uint64_t c0 = 0; rc == CLS_OK && c0 < C.cells; c0 += tile)
        rc = diff_tile(e, C, c0, uint32_t(std::min(tile, C.cells - c0)));
    if (rc == CLS_OK) rc = diff_outputs(e, C);
    if (rc != CLS_OK) return rc;
    if (out->n_cells) *out->n_cells = C.cells;
    if (out->dims) {
        out->dims[0] = C.Ks; out->dims[1] = C.Kd; out->dims[2] = C.Kt; out->dims[3] = C.Ku;
    }
    return CLS_OK;
}
