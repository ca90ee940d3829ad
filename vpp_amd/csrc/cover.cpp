// cls_table_cover (include/contivcls.h): which rules of one table no packet
// terminates at, and for every other rule the least packet that does.
// evalACL sees a packet in its source address (Contains tests of source
// networks), its destination address (of destination networks), its protocol
// and its destination port (comparisons with the range ends of that protocol's
// section), so the terminating rule is constant on every cell of source class
// x destination class x (protocol, port class) column.  The Ks Kd T cells, cell
// = (s Kd + d) T + j, go through in tiles of cover_tile cells: per tile the
// expand launch (k_cover.hip), classify_rules_locked unchanged (engine.cpp:
// what cls_classify_rules runs for a device batch), then the fold launch; one
// finish launch at the end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/contivcls.h"
#include "engine_int.hpp"
#include "goparse.hpp"
#include "kernels.hpp"

static_assert(sizeof(cls_cover_witness) == 16, "cls_cover_witness is 16 bytes");

constexpr uint64_t kCoverMaxCells = 1ull << 40;

std::vector<uint32_t> cover_side_starts(const cls_rule* rules, uint32_t n, uint32_t side) {
    std::vector<uint32_t> v{0};
    for (uint32_t i = 0; i < n; ++i) {
        const char* str = side ? rules[i].dst_network : rules[i].src_network;
        if (!str) continue;
        const Prefix p = parse_cidr(str);
        if (p.fam != 4 || p.len < 0 || p.len > 32) continue;   // a parse error, or family 16: no IPv4 address
        const uint32_t lo = uint32_t(p.addr[0]) << 24 | uint32_t(p.addr[1]) << 16 | uint32_t(p.addr[2]) << 8 | p.addr[3];
        const uint32_t hi = lo | (p.len ? uint32_t((1ull << (32 - p.len)) - 1) : 0xFFFFFFFFu);
        v.push_back(lo);
        if (hi != 0xFFFFFFFFu) v.push_back(hi + 1);
    }
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}

extern "C" int cls_cover_classes(const cls_rule* rules, uint32_t n_rules, uint32_t side, uint32_t* lo_out,
                                 uint32_t cap, uint32_t* n) {
    if (!n || side > 1 || (n_rules && !rules)) return CLS_E_INVAL;
    const std::vector<uint32_t> v = cover_side_starts(rules, n_rules, side);
    *n = uint32_t(v.size());
    if (lo_out && cap >= v.size()) std::copy(v.begin(), v.end(), lo_out);
    return CLS_OK;
}

namespace {

// The call's resolved arguments.
struct CoverCall {
    std::shared_ptr<Table> t;
    uint32_t table_id = 0;
    bool k16 = false, linear = false, dev = false;
    uint32_t Ks = 0, Kd = 0, Kt = 0, Ku = 0, T = 0;
    uint64_t cells = 0, tile = 0;
    size_t off_dlo = 0, off_col = 0, tab_bytes = 0;   // in the class tables' blob, behind the source starts
    cls_cover_out o{};
    hipStream_t s = nullptr;
    uint32_t n_out() const { return t->n_rules + 1; }
};

// Checks everything a refusal can depend on: no device work is queued, and no
// output written, before this returns CLS_OK.
int cover_inputs(cls_engine* e, uint32_t table_id, uint32_t af, const cls_cover_out* o, uint32_t flags, void* stream,
                 CoverCall& C) {
    const auto it = e->tables.find(table_id);
    if (it == e->tables.end()) return fail(e, CLS_E_NOTFOUND, "no table %u", table_id);
    C.t = it->second;
    C.table_id = table_id;
    if (af != CLS_AF_V4 && af != CLS_AF_V16) return fail(e, CLS_E_INVAL, "af must be CLS_AF_V4 or CLS_AF_V16");
    if (af == CLS_AF_V16 && !C.t->p16.ok)
        return fail(e, CLS_E_INVAL, "no 16-byte classifier for this table: %s", C.t->p16.why.c_str());
    if (flags & ~uint32_t(CLS_F_DEVICE | CLS_F_FORCE_LINEAR))
        return fail(e, CLS_E_INVAL, "table cover takes CLS_F_DEVICE and CLS_F_FORCE_LINEAR only");
    if (!o->live_out && !o->witness_out && !o->cells_out && !o->n_dead)
        return fail(e, CLS_E_INVAL, "table cover without live_out, witness_out, cells_out or n_dead");
    C.dev = flags & CLS_F_DEVICE;
    if (C.dev && (!aligned(o->witness_out, 16) || !aligned(o->cells_out, 8) || !aligned(o->n_dead, 4)))
        return fail(e, CLS_E_INVAL, "device table cover: witness_out 16-byte, cells_out 8-byte, n_dead 4-byte aligned");
    C.linear = flags & CLS_F_FORCE_LINEAR;
    // the linear kernel is the IPv4 one: the sweep's 16-byte packets are
    // IPv4-mapped, which it evaluates as the IPv4 packets they are
    C.k16 = af == CLS_AF_V16 && !C.linear;
    C.Ks = uint32_t(C.t->cover_lo[0].size());
    C.Kd = uint32_t(C.t->cover_lo[1].size());
    C.Kt = uint32_t(C.t->port_lo[0].size());
    C.Ku = uint32_t(C.t->port_lo[1].size());
    C.T = C.Kt + C.Ku + 2;                                  // <= 2^17 + 2
    const uint64_t pairs = uint64_t(C.Ks) * C.Kd;           // each below 2^32: no overflow
    if (pairs > kCoverMaxCells / C.T || pairs * C.T > kCoverMaxCells)
        return fail(e, CLS_E_INVAL, "table cover above 2^40 cells (Ks %u source classes x Kd %u destination classes x "
                                    "T %u columns)", C.Ks, C.Kd, C.T);
    C.cells = pairs * C.T;
    C.tile = e->opts.cover_tile;
    C.s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    C.o = *o;
    C.off_dlo = (size_t(C.Ks) * 4 + 15) & ~size_t(15);
    C.off_col = (C.off_dlo + size_t(C.Kd) * 4 + 15) & ~size_t(15);
    C.tab_bytes = C.off_col + ((size_t(C.T) * 4 + 15) & ~size_t(15));
    return CLS_OK;
}

// The three class tables in one blob: source starts, destination starts, the
// columns (dport | proto << 16; protocol 3 stands for every value above 2).
int cover_upload(cls_engine* e, const CoverCall& C) {
    std::vector<uint8_t>& up = e->cover_up;                  // outlives the unsynchronised upload
    up.assign(C.tab_bytes, 0);
    std::memcpy(up.data(), C.t->cover_lo[0].data(), size_t(C.Ks) * 4);
    std::memcpy(up.data() + C.off_dlo, C.t->cover_lo[1].data(), size_t(C.Kd) * 4);
    uint32_t* col = reinterpret_cast<uint32_t*>(up.data() + C.off_col);
    for (uint32_t p = 0; p < 2; ++p)
        for (uint16_t lo : C.t->port_lo[p]) *col++ = uint32_t(lo) | p << 16;
    *col++ = uint32_t(CLS_PROTO_ICMP) << 16;
    *col++ = 3u << 16;
    HIPC(e, e->v_tab.ensure(C.tab_bytes));
    HIPC(e, hipMemcpyAsync(e->v_tab.p, up.data(), C.tab_bytes, hipMemcpyHostToDevice, C.s));
    return CLS_OK;
}

// A tile's arrays (whole groups of four cells: the tile rounded up to 1024),
// the accumulators, and whatever output the caller does not take on the device.
int cover_scratch(cls_engine* e, const CoverCall& C) {
    const size_t n = size_t((std::min(C.tile, C.cells) + 1023) & ~uint64_t(1023)), r = C.n_out();
    HIPC(e, e->v_src.ensure(n * (C.k16 ? 16 : 4)));
    HIPC(e, e->v_dst.ensure(n * (C.k16 ? 16 : 4)));
    HIPC(e, e->v_dport.ensure(n * 2));
    HIPC(e, e->v_proto.ensure(n));
    HIPC(e, e->v_rule.ensure(n * 4));
    HIPC(e, e->v_min.ensure(r * 8));
    HIPC(e, hipMemsetAsync(e->v_min.p, 0xFF, r * 8, C.s));
    if (!C.dev || !C.o.cells_out) HIPC(e, e->v_cnt.ensure(r * 8));
    if (!C.dev && C.o.witness_out) HIPC(e, e->v_wit.ensure(r * 16));
    if (!C.dev && C.o.live_out) HIPC(e, e->v_live.ensure(r));
    if (!C.dev && C.o.n_dead) HIPC(e, e->v_dead.ensure(4));
    return CLS_OK;
}

unsigned long long* cover_cnt(cls_engine* e, const CoverCall& C) {
    return C.dev && C.o.cells_out ? reinterpret_cast<unsigned long long*>(C.o.cells_out)
                                  : e->v_cnt.as<unsigned long long>();
}

CoverTile cover_tile_of(cls_engine* e, const CoverCall& C, uint64_t c0, uint32_t n) {
    const uint8_t* tab = e->v_tab.as<uint8_t>();
    return CoverTile{c0, n, C.Kd, C.T, reinterpret_cast<const uint32_t*>(tab),
                     reinterpret_cast<const uint32_t*>(tab + C.off_dlo),
                     reinterpret_cast<const uint32_t*>(tab + C.off_col)};
}

// One tile: the n cells from c0 on.
int cover_tile(cls_engine* e, const CoverCall& C, uint64_t c0, uint32_t n) {
    HIPC(e, launch_cover_expand(cover_tile_of(e, C, c0, n), C.k16, e->v_src.p, e->v_dst.p, e->v_dport.as<uint16_t>(),
                                e->v_proto.as<uint8_t>(), e->n_cu, C.s));
    // the evaluator, unchanged: the matched-rule trace of a device batch
    cls_pkt_soa pk{};
    pk.af = C.k16 ? CLS_AF_V16 : CLS_AF_V4;
    if (C.k16) {
        pk.src16 = e->v_src.as<uint8_t>(); pk.dst16 = e->v_dst.as<uint8_t>();
    } else {
        pk.src4 = e->v_src.as<uint32_t>(); pk.dst4 = e->v_dst.as<uint32_t>();
    }
    pk.dport = e->v_dport.as<uint16_t>();
    pk.proto = e->v_proto.as<uint8_t>();
    const int rc = classify_rules_locked(e, C.table_id, &pk, n, nullptr, e->v_rule.as<uint32_t>(), CLS_F_DEVICE, C.s,
                                         C.linear);
    if (rc != CLS_OK) return rc;
    HIPC(e, launch_cover_fold(c0, n, e->v_rule.as<uint32_t>(), C.n_out(), e->v_min.as<unsigned long long>(),
                              cover_cnt(e, C), e->n_cu, C.s));
    return CLS_OK;
}

// The finish launch into the caller's device memory, or into the engine's and
// from there to the caller's host arrays.  A device call is stream-ordered
// (conn_last).
int cover_outputs(cls_engine* e, const CoverCall& C) {
    const uint32_t r = C.n_out();
    uint8_t* live = !C.o.live_out ? nullptr : C.dev ? C.o.live_out : e->v_live.as<uint8_t>();
    uint4* wit = !C.o.witness_out ? nullptr
                 : C.dev          ? reinterpret_cast<uint4*>(C.o.witness_out)
                                  : e->v_wit.as<uint4>();
    uint32_t* dead = !C.o.n_dead ? nullptr : C.dev ? C.o.n_dead : e->v_dead.as<uint32_t>();
    if (dead) HIPC(e, hipMemsetAsync(dead, 0, 4, C.s));
    if (live || wit || dead)
        HIPC(e, launch_cover_finish(cover_tile_of(e, C, 0, 0), e->v_min.as<unsigned long long>(), r, live, wit, dead,
                                    C.s));
    if (C.dev) {
        e->conn_last = C.s;
        return CLS_OK;
    }
    const hipMemcpyKind kind = hipMemcpyDeviceToHost;
    if (live) HIPC(e, hipMemcpyAsync(C.o.live_out, live, r, kind, C.s));
    if (wit) HIPC(e, hipMemcpyAsync(C.o.witness_out, wit, size_t(r) * 16, kind, C.s));
    if (dead) HIPC(e, hipMemcpyAsync(C.o.n_dead, dead, 4, kind, C.s));
    if (C.o.cells_out) HIPC(e, hipMemcpyAsync(C.o.cells_out, e->v_cnt.p, size_t(r) * 8, kind, C.s));
    HIPC(e, hipStreamSynchronize(C.s));
    return CLS_OK;
}

}  // namespace

extern "C" int cls_table_cover(cls_engine* e, uint32_t table_id, uint32_t af, const cls_cover_out* out,
                               uint32_t flags, void* stream) {
    if (!e) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    if (!out) return fail(e, CLS_E_INVAL, "table cover without outputs");
    CoverCall C;
    int rc = cover_inputs(e, table_id, af, out, flags, stream, C);
    if (rc != CLS_OK) return rc;
    HIPC(e, hipSetDevice(e->device));
    rc = conn_quiesce(e);        // an earlier stream-ordered call may still use the scratch
    if (rc == CLS_OK) rc = cover_upload(e, C);
    if (rc == CLS_OK) rc = cover_scratch(e, C);
    if (rc == CLS_OK) rc = hipMemsetAsync(cover_cnt(e, C), 0, size_t(C.n_out()) * 8, C.s) == hipSuccess
                               ? CLS_OK
                               : fail(e, CLS_E_HIP, "table cover: clearing the cell counts failed");
    for (uint64_t c0 = 0; rc == CLS_OK && c0 < C.cells; c0 += C.tile)
        rc = cover_tile(e, C, c0, uint32_t(std::min(C.tile, C.cells - c0)));
    if (rc == CLS_OK) rc = cover_outputs(e, C);
    if (rc != CLS_OK) return rc;
    if (out->n_cells) *out->n_cells = C.cells;
    if (out->dims) {
        out->dims[0] = C.Ks; out->dims[1] = C.Kd; out->dims[2] = C.Kt; out->dims[3] = C.Ku;
    }
    return CLS_OK;
}
