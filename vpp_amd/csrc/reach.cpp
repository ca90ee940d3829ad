// The reachability matrix (cls_reach_matrix): testConnection over every
// (probe, source, destination) cell of N endpoints x P probes, evaluated on
// the device from the endpoint and probe lists -- the rows a connection batch
// would need are never materialised by the caller.  The call as a sequence of
// stages: its arguments (ReachCall), the endpoint / probe tables' upload, the
// tile scratch, then per tile of at most reach_tile connections the expand
// launch (k_reach.hip), connect_locked on the expanded device batch, the
// reduce launch and a host call's copy back; at the end the accumulators'
// copy to the outputs.  cls_reach_diff is the same call with a baseline: per
// tile it adds the diff launches (k_reach_diff.hip) behind the reduce launch,
// and its own outputs at the end.  cls_reach_ports and cls_reach_hops, on the
// same tile pipeline and scratch, have their sections below, and
// cls_reach_external behind cls_reach_ports.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/contivcls.h"
#include "engine_int.hpp"
#include "goparse.hpp"
#include "kernels.hpp"
#include "reach_classes.hpp"

using namespace cls;

constexpr uint64_t kReachMaxCells = 1ull << 36;   // P x N x N of one call

// cls_reach_classes: what one pass over the matrix launches per tile -- the
// fold into the sums, the diagonal and the mask, or the verify against the
// table of the candidate classes.
struct ClassPass {
    bool verify = false;
    uint64_t seed_r = 0, seed_c = 0;
    unsigned long long* sums = nullptr;
    uint8_t* diag = nullptr;
    uint32_t* mask = nullptr;
    const uint32_t* cls = nullptr;
    uint32_t C = 0;
    uint32_t *tab = nullptr, *bad = nullptr;
};

// The call's resolved arguments.
struct ReachCall {
    bool k16 = false, dev = false;
    uint32_t N = 0, P = 0;
    uint64_t cells = 0;                    // P x N x N
    uint64_t tile = 0;                     // connections per tile (a multiple of 1024)
    uint32_t mode = 0;                     // the evaluator's flags (CLS_F_COUNT / CONN_CLS / FORCE_LINEAR)
    hipStream_t s = nullptr;
    uint8_t* verdict_out = nullptr;
    uint64_t* hist_out = nullptr;
    uint32_t* allow_out = nullptr;
    bool reduce() const { return hist_out || allow_out; }
    // cls_reach_diff: the baseline (null: cls_reach_matrix) and its outputs;
    // inplace: verdict_out == base
    const uint8_t* base = nullptr;
    bool inplace = false;
    cls_reach_change* changes = nullptr;
    uint64_t cap = 0;
    uint64_t* n_changes = nullptr;
    uint64_t* trans_out = nullptr;
    uint32_t* changed_out = nullptr;
    // cls_reach_hops: the adjacency bitmap every tile's ALLOW cells are folded into
    unsigned long long* adj = nullptr;
    // cls_reach_classes: the pass every tile's cells go through
    const ClassPass* cpass = nullptr;
    // the chunk counts and their scan: for the records, the total, and a
    // device call's in-place stores (made by the emit launch)
    bool scan() const { return changes || n_changes || (dev && inplace); }
    // the tables' blob (r_tab / reach_up): interface ids at 0, addresses, probes
    size_t off_addr = 0, off_probe = 0, tab_bytes = 0;
};

// A reach scratch buffer grows only once the last stream-ordered batch has
// finished with it (the rule of the connection scratch).
static hipError_t reach_grow(cls_engine* e, DevBuf& d, size_t bytes) {
    if (bytes > d.bytes && conn_quiesce(e) != CLS_OK) return hipErrorUnknown;
    return d.ensure(bytes);
}

// The endpoint arrays of `spec` (the probes' arrays are the caller's to check).
static int reach_spec(cls_engine* e, const cls_reach_spec* sp, ReachCall& R) {
    R.k16 = sp->af == CLS_AF_V16;
    if (!R.k16 && sp->af != CLS_AF_V4) return fail(e, CLS_E_INVAL, "af must be CLS_AF_V4 or CLS_AF_V16");
    if (!sp->n_endpoints || !sp->n_probes) return fail(e, CLS_E_INVAL, "reach matrix without endpoints or probes");
    if (!sp->if_id || !(R.k16 ? static_cast<const void*>(sp->addr16) : sp->addr4) || !sp->proto || !sp->sport)
        return fail(e, CLS_E_INVAL, "missing reach matrix arrays");
    return CLS_OK;
}
static int reach_spec_ifs(cls_engine* e, const cls_reach_spec* sp) {
    const uint32_t n_ifs = uint32_t(e->if_acl.size());
    for (uint32_t i = 0; i < sp->n_endpoints; ++i)
        if (sp->if_id[i] >= n_ifs) return fail(e, CLS_E_INVAL, "endpoint %u: unknown interface id", i);
    return CLS_OK;
}

// N, P and the cell bound.
static int reach_cells(cls_engine* e, const cls_reach_spec* sp, ReachCall& R) {
    R.N = sp->n_endpoints;
    R.P = sp->n_probes;
    // (N^2 first: P x N^2 <= 2^36 with P >= 1 needs N <= 2^18)
    if (R.N > (1u << 18) || uint64_t(R.N) * R.N > kReachMaxCells / R.P)
        return fail(e, CLS_E_INVAL, "reach matrix above 2^36 cells");
    R.cells = uint64_t(R.N) * R.N * R.P;
    return CLS_OK;
}
// The evaluator's flags, the tile, the stream and the tables' layout of a
// call whose arguments passed.
static void reach_resolve(cls_engine* e, uint32_t flags, void* stream, ReachCall& R) {
    R.mode = flags & (CLS_F_COUNT | CLS_F_CONN_CLS | CLS_F_FORCE_LINEAR);
    R.tile = e->opts.reach_tile;
    R.s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    R.off_addr = (size_t(R.N) * 4 + 15) & ~size_t(15);
    R.off_probe = R.off_addr + size_t(R.N) * (R.k16 ? 16 : 4);
    R.off_probe = (R.off_probe + 15) & ~size_t(15);
    R.tab_bytes = R.off_probe + size_t(R.P) * sizeof(uint2);
}

// Checks everything a refusal can depend on: no device work is queued before
// this returns CLS_OK.
static int reach_inputs(cls_engine* e, const cls_reach_spec* sp, uint8_t* verdict_out, uint64_t* hist_out,
                        uint32_t* allow_out, uint32_t flags, void* stream, ReachCall& R) {
    int rc = reach_spec(e, sp, R);
    if (rc != CLS_OK) return rc;
    if (!sp->dport) return fail(e, CLS_E_INVAL, "missing reach matrix arrays");
    // (a diff has outputs of its own, and its verdict_out may simply be NULL)
    if (!R.base && !verdict_out && !hist_out && !allow_out)
        return fail(e, CLS_E_INVAL, "reach matrix without an output");
    if (!R.base && !verdict_out && !(flags & CLS_F_NO_VERDICT))
        return fail(e, CLS_E_INVAL, "verdict_out is NULL without CLS_F_NO_VERDICT");
    rc = reach_cells(e, sp, R);
    if (rc != CLS_OK) return rc;
    R.dev = flags & CLS_F_DEVICE;
    if (R.dev && (!aligned(verdict_out, 16) || !aligned(hist_out, 8) || !aligned(allow_out, 4)))
        return fail(e, CLS_E_INVAL, "device outputs: verdict_out 16-byte, hist_out 8-byte, allow_out 4-byte aligned");
    rc = reach_spec_ifs(e, sp);
    if (rc != CLS_OK) return rc;
    R.verdict_out = verdict_out;
    R.hist_out = hist_out;
    R.allow_out = allow_out;
    reach_resolve(e, flags, stream, R);
    return CLS_OK;
}

// What cls_reach_diff refuses beyond reach_inputs (which ran: R.cells, R.dev).
static int reach_diff_inputs(cls_engine* e, const cls_reach_diff_out* o, ReachCall& R) {
    if (!o->changes && !o->n_changes && !o->trans_out && !o->changed_out)
        return fail(e, CLS_E_INVAL, "reach diff without changes, n_changes, trans_out or changed_out");
    if (o->changes && !o->n_changes) return fail(e, CLS_E_INVAL, "reach diff: changes without n_changes");
    if (o->changes && !o->cap) return fail(e, CLS_E_INVAL, "reach diff: changes with cap 0");
    if (R.dev && (!aligned(R.base, 16) || !aligned(o->changes, 16) || !aligned(o->n_changes, 8) ||
                  !aligned(o->trans_out, 8) || !aligned(o->changed_out, 4)))
        return fail(e, CLS_E_INVAL, "device reach diff: base, changes 16-byte, n_changes, trans_out 8-byte, "
                                    "changed_out 4-byte aligned");
    R.inplace = R.verdict_out == R.base;
    if (R.verdict_out && !R.inplace) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(R.base), b = reinterpret_cast<uintptr_t>(R.verdict_out);
        if (a < b + R.cells && b < a + R.cells)
            return fail(e, CLS_E_INVAL, "reach diff: verdict_out overlaps base without being equal to it");
    }
    R.changes = o->changes;
    R.cap = o->changes ? o->cap : 0;
    R.n_changes = o->n_changes;
    R.trans_out = o->trans_out;
    R.changed_out = o->changed_out;
    return CLS_OK;
}

// Orders the call behind the last stream-ordered batch of another stream,
// which may still use the scratch.
static int reach_follow(cls_engine* e, const ReachCall& R) {
    HIPC(e, hipSetDevice(e->device));
    if (e->conn_last && e->conn_last != R.s) {
        if (!e->conn_sync_ev) HIPC(e, hipEventCreateWithFlags(&e->conn_sync_ev, hipEventDisableTiming));
        HIPC(e, hipEventRecord(e->conn_sync_ev, e->conn_last));
        HIPC(e, hipStreamWaitEvent(R.s, e->conn_sync_ev, 0));
    }
    return CLS_OK;
}

// The call's tables (one blob), uploaded once per call from the engine's copy
// (the caller's arrays are not read after this); nothing is copied when the
// last call's blob is the same.  The call's first device work (reach_follow).
static int reach_upload_tab(cls_engine* e, const ReachCall& R, std::vector<uint8_t>& tab) {
    const int frc = reach_follow(e, R);
    if (frc != CLS_OK) return frc;
    const void* was = e->r_tab.p;
    HIPC(e, reach_grow(e, e->r_tab, tab.size()));
    if (e->r_tab.p == was && e->reach_up == tab) return CLS_OK;
    const int rc = conn_quiesce(e);                  // an earlier copy may still read reach_up
    if (rc != CLS_OK) return rc;
    e->reach_up.swap(tab);
    HIPC(e, hipMemcpyAsync(e->r_tab.p, e->reach_up.data(), e->reach_up.size(), hipMemcpyHostToDevice, R.s));
    return CLS_OK;
}

// The endpoint and probe tables.
static int reach_upload(cls_engine* e, const cls_reach_spec* sp, const ReachCall& R) {
    std::vector<uint8_t> tab(R.tab_bytes, 0);
    std::memcpy(tab.data(), sp->if_id, size_t(R.N) * 4);
    std::memcpy(tab.data() + R.off_addr, R.k16 ? static_cast<const void*>(sp->addr16) : sp->addr4,
                size_t(R.N) * (R.k16 ? 16 : 4));
    uint2* pr = reinterpret_cast<uint2*>(tab.data() + R.off_probe);
    for (uint32_t p = 0; p < R.P; ++p) pr[p] = uint2{uint32_t(sp->sport[p]) | uint32_t(sp->dport[p]) << 16, sp->proto[p]};
    return reach_upload_tab(e, R, tab);
}

// The tile's arrays (whole groups of four connections), the verdict bytes
// when the evaluator cannot write the caller's, the accumulators (cleared).
static int reach_scratch(cls_engine* e, const ReachCall& R) {
    const size_t n = size_t((std::min(R.tile, R.cells) + 3) & ~uint64_t(3)), ab = R.k16 ? 16 : 4;
    HIPC(e, reach_grow(e, e->r_src, n * ab)); HIPC(e, reach_grow(e, e->r_dst, n * ab));
    HIPC(e, reach_grow(e, e->r_sif, n * 4)); HIPC(e, reach_grow(e, e->r_dif, n * 4));
    HIPC(e, reach_grow(e, e->r_sport, n * 2)); HIPC(e, reach_grow(e, e->r_dport, n * 2));
    HIPC(e, reach_grow(e, e->r_proto, n));
    if (!R.dev || !R.verdict_out || R.inplace) HIPC(e, reach_grow(e, e->r_verdict, n));
    if (R.hist_out) {
        HIPC(e, reach_grow(e, e->r_hist, size_t(R.P) * 4 * 8));
        HIPC(e, hipMemsetAsync(e->r_hist.p, 0, size_t(R.P) * 4 * 8, R.s));
    }
    if (R.allow_out) {
        HIPC(e, reach_grow(e, e->r_allow, size_t(R.P) * R.N * 4));
        HIPC(e, hipMemsetAsync(e->r_allow.p, 0, size_t(R.P) * R.N * 4, R.s));
    }
    return CLS_OK;
}

// The diff's scratch: a host call's tile of baseline bytes and its records
// (min(cap, P N^2) of them), the tile's chunk counts and first indices, the
// running total and the accumulators (cleared).
static int reach_diff_scratch(cls_engine* e, const ReachCall& R) {
    const size_t n = size_t((std::min(R.tile, R.cells) + 3) & ~uint64_t(3));
    if (!R.dev) HIPC(e, reach_grow(e, e->r_base, n));
    if (!R.dev && R.changes)
        HIPC(e, reach_grow(e, e->r_changes, size_t(std::min(R.cap, R.cells)) * sizeof(cls_reach_change)));
    if (R.scan()) {
        const size_t chunks = (n + kReachChunk - 1) / kReachChunk;
        HIPC(e, reach_grow(e, e->r_dcount, chunks * 4));
        HIPC(e, reach_grow(e, e->r_dbase, chunks * 8));
        HIPC(e, reach_grow(e, e->r_dtotal, 8));
        HIPC(e, hipMemsetAsync(e->r_dtotal.p, 0, 8, R.s));
    }
    if (R.trans_out) {
        HIPC(e, reach_grow(e, e->r_trans, size_t(R.P) * 16 * 8));
        HIPC(e, hipMemsetAsync(e->r_trans.p, 0, size_t(R.P) * 16 * 8, R.s));
    }
    if (R.changed_out) {
        HIPC(e, reach_grow(e, e->r_changed, size_t(R.P) * R.N * 4));
        HIPC(e, hipMemsetAsync(e->r_changed.p, 0, size_t(R.P) * R.N * 4, R.s));
    }
    return CLS_OK;
}

// The tile's verdicts v against its baseline bytes: count, then -- for the
// records, the total or an in-place call's stores -- scan and emit.  A host
// call's baseline tile goes up into scratch first.
static int reach_diff_tile(cls_engine* e, const ReachCall& R, const ReachTile& T, uint64_t first, uint64_t row,
                           const uint8_t* v) {
    const uint8_t* base = R.base + first;
    if (!R.dev) {
        HIPC(e, hipMemcpyAsync(e->r_base.p, base, T.n, hipMemcpyHostToDevice, R.s));
        base = e->r_base.as<uint8_t>();
    }
    uint32_t* count = R.scan() ? e->r_dcount.as<uint32_t>() : nullptr;
    HIPC(e, launch_reach_diff_count(T, base, v, count,
                                    R.trans_out ? e->r_trans.as<unsigned long long>() + 16 * uint64_t(T.p0) : nullptr,
                                    R.changed_out ? e->r_changed.as<uint32_t>() + row : nullptr, e->n_cu, R.s));
    if (!R.scan()) return CLS_OK;
    unsigned long long* at = e->r_dbase.as<unsigned long long>();
    HIPC(e, launch_reach_diff_scan((T.n + kReachChunk - 1) / kReachChunk, count, at,
                                   e->r_dtotal.as<unsigned long long>(), R.s));
    // the caller's device records, or the engine's (the cells past the buffer's
    // min(cap, P N^2) records are past cap)
    cls_reach_change* rec = R.dev ? R.changes : R.changes ? e->r_changes.as<cls_reach_change>() : nullptr;
    HIPC(e, launch_reach_diff_emit(T, base, v, count, at, reinterpret_cast<uint4*>(rec), R.cap,
                                   R.dev && R.inplace ? R.verdict_out + first : nullptr, e->n_cu, R.s));
    return CLS_OK;
}

// The tile's launch of a cls_reach_classes pass over its verdict bytes v.
static hipError_t class_launch(const ClassPass& c, const ReachTile& T, const uint8_t* v, hipStream_t s) {
    return c.verify ? launch_reach_class_verify(T, v, c.cls, c.C, c.tab, c.bad, s)
                    : launch_reach_class_fold(T, v, c.seed_r, c.seed_c, c.sums, c.diag, c.mask, s);
}

// One tile: cells [first, first + n) of the matrix.
static int reach_tile(cls_engine* e, const ReachCall& R, uint64_t first, uint32_t n) {
    const uint64_t row = first / R.N;                 // (probe, source) row of the first cell
    const ReachTile T{R.N, uint32_t(row / R.N), uint32_t(row % R.N), uint32_t(first % R.N), n};
    const uint8_t* tab = e->r_tab.as<uint8_t>();
    ReachExpand X{};
    X.ep_if = reinterpret_cast<const uint32_t*>(tab);
    X.ep_addr = tab + R.off_addr;
    X.probe = reinterpret_cast<const uint2*>(tab + R.off_probe);
    X.src_if = e->r_sif.as<uint32_t>(); X.dst_if = e->r_dif.as<uint32_t>();
    X.src = e->r_src.p; X.dst = e->r_dst.p;
    X.sport = e->r_sport.as<uint16_t>(); X.dport = e->r_dport.as<uint16_t>();
    X.proto = e->r_proto.as<uint8_t>();
    HIPC(e, launch_reach_expand(T, X, R.k16, e->n_cu, R.s));
    // the evaluator, unchanged: a device batch over the expanded arrays,
    // straight into a device verdict_out
    cls_conn_soa c{};
    c.pkt.af = R.k16 ? CLS_AF_V16 : CLS_AF_V4;
    if (R.k16) {
        c.pkt.src16 = e->r_src.as<uint8_t>(); c.pkt.dst16 = e->r_dst.as<uint8_t>();
    } else {
        c.pkt.src4 = e->r_src.as<uint32_t>(); c.pkt.dst4 = e->r_dst.as<uint32_t>();
    }
    c.pkt.sport = X.sport; c.pkt.dport = X.dport; c.pkt.proto = X.proto;
    c.src_if = X.src_if; c.dst_if = X.dst_if;
    // (an in-place diff's verdicts reach the matrix behind the compare)
    uint8_t* v = R.dev && R.verdict_out && !R.inplace ? R.verdict_out + first : e->r_verdict.as<uint8_t>();
    const int rc = connect_locked(e, &c, n, v, CLS_F_DEVICE | R.mode, R.s, false);
    if (rc != CLS_OK) return rc;
    if (R.reduce())
        HIPC(e, launch_reach_reduce(T, v, R.hist_out ? e->r_hist.as<unsigned long long>() + 4 * uint64_t(T.p0) : nullptr,
                                    R.allow_out ? e->r_allow.as<uint32_t>() + row : nullptr, e->n_cu, R.s));
    if (R.adj) HIPC(e, launch_reach_adj_fold(T, v, R.adj, e->n_cu, R.s));
    if (R.cpass) HIPC(e, class_launch(*R.cpass, T, v, R.s));
    if (R.base) {
        const int drc = reach_diff_tile(e, R, T, first, row, v);
        if (drc != CLS_OK) return drc;
    }
    if (!R.dev && R.verdict_out) HIPC(e, hipMemcpyAsync(R.verdict_out + first, v, n, hipMemcpyDeviceToHost, R.s));
    return CLS_OK;
}

// The diff's accumulators and total to the caller's outputs; a host call
// waits for the total and copies that many of its records (none past them).
static int reach_diff_outputs(cls_engine* e, const ReachCall& R) {
    const hipMemcpyKind kind = R.dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (R.trans_out) HIPC(e, hipMemcpyAsync(R.trans_out, e->r_trans.p, size_t(R.P) * 16 * 8, kind, R.s));
    if (R.changed_out) HIPC(e, hipMemcpyAsync(R.changed_out, e->r_changed.p, size_t(R.P) * R.N * 4, kind, R.s));
    if (!R.n_changes) return CLS_OK;
    if (R.dev) {
        HIPC(e, hipMemcpyAsync(R.n_changes, e->r_dtotal.p, 8, kind, R.s));
        return CLS_OK;
    }
    uint64_t total = 0;
    HIPC(e, hipMemcpyAsync(&total, e->r_dtotal.p, 8, kind, R.s));
    HIPC(e, hipStreamSynchronize(R.s));
    const uint64_t n = std::min(total, R.cap);
    if (R.changes && n) {
        HIPC(e, hipMemcpyAsync(R.changes, e->r_changes.p, size_t(n) * sizeof(cls_reach_change), kind, R.s));
        HIPC(e, hipStreamSynchronize(R.s));
    }
    *R.n_changes = total;
    return CLS_OK;
}

// The accumulators to the caller's outputs; a host call returns with its
// results, a device call is stream-ordered (conn_last).
static int reach_outputs(cls_engine* e, const ReachCall& R) {
    const hipMemcpyKind kind = R.dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (R.hist_out) HIPC(e, hipMemcpyAsync(R.hist_out, e->r_hist.p, size_t(R.P) * 4 * 8, kind, R.s));
    if (R.allow_out) HIPC(e, hipMemcpyAsync(R.allow_out, e->r_allow.p, size_t(R.P) * R.N * 4, kind, R.s));
    if (!R.dev) {
        HIPC(e, hipStreamSynchronize(R.s));
        e->conn_last = nullptr;
    } else {
        e->conn_last = R.s;
    }
    return CLS_OK;
}

extern "C" int cls_reach_matrix(cls_engine* e, const cls_reach_spec* spec, uint8_t* verdict_out, uint64_t* hist_out,
                                uint32_t* allow_out, uint32_t flags, void* stream) {
    if (!e || !spec) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    ReachCall R;
    int rc = reach_inputs(e, spec, verdict_out, hist_out, allow_out, flags, stream, R);
    if (rc == CLS_OK) rc = reach_upload(e, spec, R);
    if (rc == CLS_OK) rc = reach_scratch(e, R);
    for (uint64_t first = 0; rc == CLS_OK && first < R.cells; first += R.tile)
        rc = reach_tile(e, R, first, uint32_t(std::min(R.tile, R.cells - first)));
    if (rc == CLS_OK) rc = reach_outputs(e, R);
    return rc;
}

extern "C" int cls_reach_diff(cls_engine* e, const cls_reach_spec* spec, const uint8_t* base,
                              const cls_reach_diff_out* out, uint32_t flags, void* stream) {
    if (!e || !spec) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    if (!base || !out) return fail(e, CLS_E_INVAL, "reach diff without a baseline or outputs");
    ReachCall R;
    R.base = base;
    int rc = reach_inputs(e, spec, out->verdict_out, out->hist_out, out->allow_out, flags, stream, R);
    if (rc == CLS_OK) rc = reach_diff_inputs(e, out, R);
    if (rc == CLS_OK) rc = reach_upload(e, spec, R);
    if (rc == CLS_OK) rc = reach_scratch(e, R);
    if (rc == CLS_OK) rc = reach_diff_scratch(e, R);
    for (uint64_t first = 0; rc == CLS_OK && first < R.cells; first += R.tile)
        rc = reach_tile(e, R, first, uint32_t(std::min(R.tile, R.cells - first)));
    if (rc == CLS_OK) rc = reach_diff_outputs(e, R);
    if (rc == CLS_OK) rc = reach_outputs(e, R);
    return rc;
}

// ---- cls_reach_ports: per-pair port ranges over all 65,536 ports ----------
// One representative port per port class (the swept protocol's rule
// boundaries over the bound ACLs) is exact, since evalACL sees the destination
// port only in comparisons with those boundaries.  The K N^2 rows are laid
// out pair-major, row = (s N + d) K + k, in tiles of whole pairs; per tile the
// expand launch (k_reach_ports.hip), connect_locked unchanged, then count,
// reach_diff_scan and emit.

std::vector<uint16_t> port_class_starts(const cls_rule* rules, uint32_t n, uint32_t proto) {
    std::vector<uint16_t> v{0};
    if (proto > uint32_t(P_UDP)) return v;            // no rule tests the port
    const bool tcp = proto == uint32_t(P_TCP);
    for (uint32_t i = 0; i < n; ++i) {
        const cls_rule& r = rules[i];
        if (!(r.flags & (tcp ? CLS_R_TCP : CLS_R_UDP)) || !(r.flags & (tcp ? CLS_R_TCP_DST : CLS_R_UDP_DST))) continue;
        // the uint16() casts of :559
        const uint16_t lo = uint16_t(tcp ? r.tcp_dst_lo : r.udp_dst_lo), hi = uint16_t(tcp ? r.tcp_dst_hi : r.udp_dst_hi);
        if (lo > hi) continue;                        // never inside [lo, hi]
        v.push_back(lo);
        if (hi != 0xFFFF) v.push_back(uint16_t(hi + 1));
    }
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}

extern "C" int cls_port_classes(const cls_rule* rules, uint32_t n_rules, uint32_t proto, uint16_t* lo_out,
                                uint32_t cap, uint32_t* n) {
    if (!n || (n_rules && !rules)) return CLS_E_INVAL;
    const std::vector<uint16_t> v = port_class_starts(rules, n_rules, proto);
    *n = uint32_t(v.size());
    if (lo_out && cap >= v.size()) std::copy(v.begin(), v.end(), lo_out);
    return CLS_OK;
}

// The call's resolved arguments: R holds the matrix's (one probe, cells =
// K N^2 rows, tile = the rows of a full tile).
struct PortsCall {
    ReachCall R;
    uint32_t K = 0, sport = 0, proto = 0;
    uint64_t pairs = 0, per_tile = 0;      // N^2; pairs per tile
    std::vector<uint16_t> lo;              // the K class starts
    size_t off_lo = 0;                     // in the tables' blob, behind the addresses
    cls_reach_ports_out o{};
    uint64_t cap = 0;                      // min(o.cap, K N^2): no index reaches K N^2
    bool scan() const { return o.ranges || o.n_ranges; }
};

// The sorted union of the class starts of the tables bound, inbound or
// outbound, to any interface of the endpoints.
static void ports_classes(cls_engine* e, const cls_reach_spec* sp, PortsCall& C) {
    C.lo.assign(1, 0);
    const uint32_t proto = sp->proto[0];
    if (proto > uint32_t(P_UDP)) return;
    std::vector<uint8_t> seen_if(e->if_acl.size(), 0);
    std::vector<int32_t> tids;
    for (uint32_t i = 0; i < sp->n_endpoints; ++i) {
        if (seen_if[sp->if_id[i]]) continue;
        seen_if[sp->if_id[i]] = 1;
        tids.push_back(e->if_acl[sp->if_id[i]].first);
        tids.push_back(e->if_acl[sp->if_id[i]].second);
    }
    std::sort(tids.begin(), tids.end());
    tids.erase(std::unique(tids.begin(), tids.end()), tids.end());
    for (int32_t tid : tids) {
        if (tid < 0) continue;
        const auto it = e->tables.find(uint32_t(tid));
        if (it == e->tables.end()) continue;
        const std::vector<uint16_t>& v = it->second->port_lo[proto];
        C.lo.insert(C.lo.end(), v.begin(), v.end());
    }
    std::sort(C.lo.begin(), C.lo.end());
    C.lo.erase(std::unique(C.lo.begin(), C.lo.end()), C.lo.end());
}

// Checks everything a refusal can depend on: no device work is queued before
// this returns CLS_OK.
static int ports_inputs(cls_engine* e, const cls_reach_spec* sp, const cls_reach_ports_out* o, uint32_t flags,
                        void* stream, PortsCall& C) {
    ReachCall& R = C.R;
    int rc = reach_spec(e, sp, R);
    if (rc != CLS_OK) return rc;
    if (sp->n_probes != 1) return fail(e, CLS_E_INVAL, "reach ports takes one probe (proto[0], sport[0])");
    if (flags & (CLS_F_COUNT | CLS_F_NO_VERDICT))
        return fail(e, CLS_E_INVAL, "reach ports evaluates representatives: no CLS_F_COUNT, no CLS_F_NO_VERDICT");
    if (!o->ranges && !o->n_ranges && !o->runs_out && !o->allow_ports_out && !o->hist_out)
        return fail(e, CLS_E_INVAL, "reach ports without ranges, n_ranges, runs_out, allow_ports_out or hist_out");
    if (o->ranges && !o->n_ranges) return fail(e, CLS_E_INVAL, "reach ports: ranges without n_ranges");
    if (o->ranges && !o->cap) return fail(e, CLS_E_INVAL, "reach ports: ranges with cap 0");
    R.dev = flags & CLS_F_DEVICE;
    if (R.dev && (!aligned(o->ranges, 16) || !aligned(o->n_ranges, 8) || !aligned(o->hist_out, 8) ||
                  !aligned(o->runs_out, 4) || !aligned(o->allow_ports_out, 4)))
        return fail(e, CLS_E_INVAL, "device reach ports: ranges 16-byte, n_ranges, hist_out 8-byte, runs_out, "
                                    "allow_ports_out 4-byte aligned");
    R.N = sp->n_endpoints;
    R.P = 1;
    if (R.N > (1u << 18)) return fail(e, CLS_E_INVAL, "reach ports above 2^36 rows (N %u)", R.N);
    rc = reach_spec_ifs(e, sp);
    if (rc != CLS_OK) return rc;
    ports_classes(e, sp, C);
    C.K = uint32_t(C.lo.size());
    C.pairs = uint64_t(R.N) * R.N;
    if (C.pairs > kReachMaxCells / C.K)
        return fail(e, CLS_E_INVAL, "reach ports above 2^36 rows (K %u classes x N %u endpoints squared)", C.K, R.N);
    R.cells = C.pairs * C.K;
    // whole pairs per tile (one when K exceeds reach_tile): no range crosses a tile
    C.per_tile = std::max<uint64_t>(1, e->opts.reach_tile / C.K);
    R.tile = C.per_tile * C.K;                        // <= max(reach_tile, 65536) <= 2^30
    R.mode = flags & (CLS_F_CONN_CLS | CLS_F_FORCE_LINEAR);
    R.s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    C.o = *o;
    C.sport = sp->sport[0];
    C.proto = sp->proto[0];
    C.cap = o->ranges ? std::min(o->cap, R.cells) : 0;
    R.off_addr = (size_t(R.N) * 4 + 15) & ~size_t(15);
    C.off_lo = (R.off_addr + size_t(R.N) * (R.k16 ? 16 : 4) + 15) & ~size_t(15);
    R.tab_bytes = C.off_lo + ((size_t(C.K) * 2 + 15) & ~size_t(15));
    if (o->n_classes) *o->n_classes = C.K;
    return CLS_OK;
}

// The endpoint table with the class starts behind it.
static int ports_upload(cls_engine* e, const cls_reach_spec* sp, const PortsCall& C) {
    const ReachCall& R = C.R;
    std::vector<uint8_t> tab(R.tab_bytes, 0);
    std::memcpy(tab.data(), sp->if_id, size_t(R.N) * 4);
    std::memcpy(tab.data() + R.off_addr, R.k16 ? static_cast<const void*>(sp->addr16) : sp->addr4,
                size_t(R.N) * (R.k16 ? 16 : 4));
    std::memcpy(tab.data() + C.off_lo, C.lo.data(), size_t(C.K) * 2);
    return reach_upload_tab(e, R, tab);
}

// Where the per-pair sums and the histogram accumulate: the caller's device
// memory, or the engine's for a host call.
static uint32_t* ports_runs(cls_engine* e, const PortsCall& C) {
    return !C.o.runs_out ? nullptr : C.R.dev ? C.o.runs_out : e->r_runs.as<uint32_t>();
}
static uint32_t* ports_allow(cls_engine* e, const PortsCall& C) {
    return !C.o.allow_ports_out ? nullptr : C.R.dev ? C.o.allow_ports_out : e->r_pallow.as<uint32_t>();
}
static unsigned long long* ports_hist(cls_engine* e, const PortsCall& C) {
    return !C.o.hist_out ? nullptr
           : C.R.dev     ? reinterpret_cast<unsigned long long*>(C.o.hist_out)
                         : e->r_phist.as<unsigned long long>();
}

// Beyond reach_scratch: a host call's records (cap of them) and sums, the
// tile's chunk counts and first indices, the running total; all cleared.
static int ports_scratch(cls_engine* e, const PortsCall& C) {
    const ReachCall& R = C.R;
    const size_t n = size_t(std::min(R.tile, R.cells)), pb = size_t(C.pairs) * 4;
    if (!R.dev) {
        if (C.o.ranges) HIPC(e, reach_grow(e, e->r_changes, size_t(C.cap) * sizeof(cls_port_range)));
        if (C.o.runs_out) HIPC(e, reach_grow(e, e->r_runs, pb));
        if (C.o.allow_ports_out) HIPC(e, reach_grow(e, e->r_pallow, pb));
        if (C.o.hist_out) HIPC(e, reach_grow(e, e->r_phist, 4 * 8));
    }
    if (C.scan()) {
        const size_t chunks = (n + kReachChunk - 1) / kReachChunk;
        HIPC(e, reach_grow(e, e->r_dcount, chunks * 4));
        HIPC(e, reach_grow(e, e->r_dbase, chunks * 8));
        HIPC(e, reach_grow(e, e->r_dtotal, 8));
        HIPC(e, hipMemsetAsync(e->r_dtotal.p, 0, 8, R.s));
    }
    if (uint32_t* p = ports_runs(e, C)) HIPC(e, hipMemsetAsync(p, 0, pb, R.s));
    if (uint32_t* p = ports_allow(e, C)) HIPC(e, hipMemsetAsync(p, 0, pb, R.s));
    if (unsigned long long* p = ports_hist(e, C)) HIPC(e, hipMemsetAsync(p, 0, 4 * 8, R.s));
    return CLS_OK;
}

// One tile: the np whole pairs from `pair` on.
static int ports_tile(cls_engine* e, const PortsCall& C, uint64_t pair, uint32_t np) {
    const ReachCall& R = C.R;
    const uint8_t* tab = e->r_tab.as<uint8_t>();
    const uint32_t n = np * C.K;
    const ReachPortsTile T{R.N, uint32_t(pair / R.N), uint32_t(pair % R.N), C.K, n,
                           reinterpret_cast<const uint16_t*>(tab + C.off_lo)};
    ReachPortsExpand X{};
    X.ep_if = reinterpret_cast<const uint32_t*>(tab);
    X.ep_addr = tab + R.off_addr;
    X.sport = C.sport;
    X.proto = C.proto;
    X.src_if = e->r_sif.as<uint32_t>(); X.dst_if = e->r_dif.as<uint32_t>();
    X.src = e->r_src.p; X.dst = e->r_dst.p;
    X.sport_out = e->r_sport.as<uint16_t>(); X.dport_out = e->r_dport.as<uint16_t>();
    X.proto_out = e->r_proto.as<uint8_t>();
    HIPC(e, launch_reach_ports_expand(T, X, R.k16, e->n_cu, R.s));
    // the evaluator, unchanged: a device batch over the expanded arrays
    cls_conn_soa c{};
    c.pkt.af = R.k16 ? CLS_AF_V16 : CLS_AF_V4;
    if (R.k16) {
        c.pkt.src16 = e->r_src.as<uint8_t>(); c.pkt.dst16 = e->r_dst.as<uint8_t>();
    } else {
        c.pkt.src4 = e->r_src.as<uint32_t>(); c.pkt.dst4 = e->r_dst.as<uint32_t>();
    }
    c.pkt.sport = X.sport_out; c.pkt.dport = X.dport_out; c.pkt.proto = X.proto_out;
    c.src_if = X.src_if; c.dst_if = X.dst_if;
    const uint8_t* v = e->r_verdict.as<uint8_t>();
    const int rc = connect_locked(e, &c, n, e->r_verdict.as<uint8_t>(), CLS_F_DEVICE | R.mode, R.s, false);
    if (rc != CLS_OK) return rc;
    uint32_t* runs = ports_runs(e, C);
    uint32_t* allow = ports_allow(e, C);
    uint32_t* count = C.scan() ? e->r_dcount.as<uint32_t>() : nullptr;
    HIPC(e, launch_reach_ports_count(T, v, count, runs ? runs + pair : nullptr, allow ? allow + pair : nullptr,
                                     ports_hist(e, C), e->n_cu, R.s));
    if (!C.scan()) return CLS_OK;
    unsigned long long* at = e->r_dbase.as<unsigned long long>();
    HIPC(e, launch_reach_diff_scan((n + kReachChunk - 1) / kReachChunk, count, at,
                                   e->r_dtotal.as<unsigned long long>(), R.s));
    cls_port_range* rec = !C.o.ranges ? nullptr : R.dev ? C.o.ranges : e->r_changes.as<cls_port_range>();
    HIPC(e, launch_reach_ports_emit(T, v, at, reinterpret_cast<uint4*>(rec), C.cap, e->n_cu, R.s));
    return CLS_OK;
}

// A host call's sums, total and records through the engine's buffers (it
// waits for the total and copies that many records, none past them); a device
// call's total.  A device call is stream-ordered (conn_last).
static int ports_outputs(cls_engine* e, const PortsCall& C) {
    const ReachCall& R = C.R;
    if (R.dev) {
        if (C.o.n_ranges) HIPC(e, hipMemcpyAsync(C.o.n_ranges, e->r_dtotal.p, 8, hipMemcpyDeviceToDevice, R.s));
        e->conn_last = R.s;
        return CLS_OK;
    }
    const hipMemcpyKind kind = hipMemcpyDeviceToHost;
    const size_t pb = size_t(C.pairs) * 4;
    if (C.o.runs_out) HIPC(e, hipMemcpyAsync(C.o.runs_out, e->r_runs.p, pb, kind, R.s));
    if (C.o.allow_ports_out) HIPC(e, hipMemcpyAsync(C.o.allow_ports_out, e->r_pallow.p, pb, kind, R.s));
    if (C.o.hist_out) HIPC(e, hipMemcpyAsync(C.o.hist_out, e->r_phist.p, 4 * 8, kind, R.s));
    uint64_t total = 0;
    if (C.o.n_ranges) HIPC(e, hipMemcpyAsync(&total, e->r_dtotal.p, 8, kind, R.s));
    HIPC(e, hipStreamSynchronize(R.s));
    const uint64_t n = std::min(total, C.cap);
    if (C.o.ranges && n) {
        HIPC(e, hipMemcpyAsync(C.o.ranges, e->r_changes.p, size_t(n) * sizeof(cls_port_range), kind, R.s));
        HIPC(e, hipStreamSynchronize(R.s));
    }
    if (C.o.n_ranges) *C.o.n_ranges = total;
    e->conn_last = nullptr;
    return CLS_OK;
}

extern "C" int cls_reach_ports(cls_engine* e, const cls_reach_spec* spec, const cls_reach_ports_out* out,
                               uint32_t flags, void* stream) {
    if (!e || !spec) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    if (!out) return fail(e, CLS_E_INVAL, "reach ports without outputs");
    PortsCall C;
    int rc = ports_inputs(e, spec, out, flags, stream, C);
    if (rc != CLS_OK) return rc;
    rc = ports_upload(e, spec, C);
    if (rc == CLS_OK) rc = reach_scratch(e, C.R);
    if (rc == CLS_OK) rc = ports_scratch(e, C);
    for (uint64_t pair = 0; rc == CLS_OK && pair < C.pairs; pair += C.per_tile)
        rc = ports_tile(e, C, pair, uint32_t(std::min(C.per_tile, C.pairs - pair)));
    if (rc == CLS_OK) rc = ports_outputs(e, C);
    return rc;
}

// ---- cls_reach_external: per-pod address ranges over all of IPv4 ----------
// The port sweep's twin over the remote address of ConnectionPodToInternet /
// ConnectionInternetToPod.  One representative address per address class (the
// parsed networks' interval ends over the bound ACLs) is exact, since evalACL
// sees the remote address only in IPNet.Contains tests of those networks.
// The D P N K rows are laid out line-major, row = ((d P + p) N + s) K + k, in
// tiles of whole lines; per tile the expand launch (k_reach_ext.hip),
// connect_locked unchanged, then count, reach_diff_scan and emit.

std::vector<uint32_t> addr_class_starts(const cls_rule* rules, uint32_t n) {
    std::vector<uint32_t> v{0};
    for (uint32_t i = 0; i < n; ++i)
        for (const char* str : {rules[i].src_network, rules[i].dst_network}) {
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

extern "C" int cls_addr_classes(const cls_rule* rules, uint32_t n_rules, uint32_t* lo_out, uint32_t cap,
                                uint32_t* n) {
    if (!n || (n_rules && !rules)) return CLS_E_INVAL;
    const std::vector<uint32_t> v = addr_class_starts(rules, n_rules);
    *n = uint32_t(v.size());
    if (lo_out && cap >= v.size()) std::copy(v.begin(), v.end(), lo_out);
    return CLS_OK;
}

// The call's resolved arguments: R holds the matrix's (cells = D P N K rows,
// tile = the rows of a full tile).
struct ExtCall {
    ReachCall R;
    uint32_t K = 0, D = 0, ext_if = 0;
    uint32_t dir_of[2] = {0, 0};           // the direction (0 egress, 1 ingress) of direction index 0, 1
    uint64_t lines = 0, per_tile = 0;      // D P N; lines per tile
    std::vector<uint32_t> lo;              // the K class starts
    size_t off_lo = 0;                     // in the tables' blob, behind the addresses and the probes
    cls_reach_ext_out o{};
    uint64_t cap = 0;                      // min(o.cap, D P N K): no index reaches D P N K
    bool scan() const { return o.ranges || o.n_ranges; }
};

// The sorted union of the class starts of the tables bound, inbound or
// outbound, to any interface of the endpoints or to ext_if.
static void ext_classes(cls_engine* e, const cls_reach_spec* sp, ExtCall& C) {
    C.lo.assign(1, 0);
    std::vector<uint8_t> seen_if(e->if_acl.size(), 0);
    std::vector<int32_t> tids;
    const auto add_if = [&](uint32_t id) {
        if (seen_if[id]) return;
        seen_if[id] = 1;
        tids.push_back(e->if_acl[id].first);
        tids.push_back(e->if_acl[id].second);
    };
    add_if(C.ext_if);
    for (uint32_t i = 0; i < sp->n_endpoints; ++i) add_if(sp->if_id[i]);
    std::sort(tids.begin(), tids.end());
    tids.erase(std::unique(tids.begin(), tids.end()), tids.end());
    for (int32_t tid : tids) {
        if (tid < 0) continue;
        const auto it = e->tables.find(uint32_t(tid));
        if (it == e->tables.end()) continue;
        const std::vector<uint32_t>& v = it->second->addr_lo;
        C.lo.insert(C.lo.end(), v.begin(), v.end());
    }
    std::sort(C.lo.begin(), C.lo.end());
    C.lo.erase(std::unique(C.lo.begin(), C.lo.end()), C.lo.end());
}

// Checks everything a refusal can depend on: no device work is queued before
// this returns CLS_OK.
static int ext_inputs(cls_engine* e, const cls_reach_spec* sp, uint32_t ext_if, uint32_t dirs,
                      const cls_reach_ext_out* o, uint32_t flags, void* stream, ExtCall& C) {
    ReachCall& R = C.R;
    int rc = reach_spec(e, sp, R);
    if (rc != CLS_OK) return rc;
    if (!sp->dport) return fail(e, CLS_E_INVAL, "missing reach matrix arrays");
    if (!dirs || (dirs & ~uint32_t(CLS_EXT_EGRESS | CLS_EXT_INGRESS)))
        return fail(e, CLS_E_INVAL, "reach external: dirs is CLS_EXT_EGRESS, CLS_EXT_INGRESS or both");
    if (flags & (CLS_F_COUNT | CLS_F_NO_VERDICT))
        return fail(e, CLS_E_INVAL, "reach external evaluates representatives: no CLS_F_COUNT, no CLS_F_NO_VERDICT");
    if (!o->ranges && !o->n_ranges && !o->runs_out && !o->allow_addrs_out && !o->hist_out)
        return fail(e, CLS_E_INVAL, "reach external without ranges, n_ranges, runs_out, allow_addrs_out or hist_out");
    if (o->ranges && !o->n_ranges) return fail(e, CLS_E_INVAL, "reach external: ranges without n_ranges");
    if (o->ranges && !o->cap) return fail(e, CLS_E_INVAL, "reach external: ranges with cap 0");
    rc = reach_cells(e, sp, R);
    if (rc != CLS_OK) return rc;
    if (R.P > 65536) return fail(e, CLS_E_INVAL, "reach external above 65536 probes (P %u)", R.P);
    R.dev = flags & CLS_F_DEVICE;
    if (R.dev && (!aligned(o->ranges, 16) || !aligned(o->n_ranges, 8) || !aligned(o->allow_addrs_out, 8) ||
                  !aligned(o->hist_out, 8) || !aligned(o->runs_out, 4)))
        return fail(e, CLS_E_INVAL, "device reach external: ranges 16-byte, n_ranges, allow_addrs_out, hist_out "
                                    "8-byte, runs_out 4-byte aligned");
    rc = reach_spec_ifs(e, sp);
    if (rc != CLS_OK) return rc;
    if (ext_if >= e->if_acl.size()) return fail(e, CLS_E_INVAL, "reach external: unknown interface id ext_if %u", ext_if);
    C.ext_if = ext_if;
    if (dirs & CLS_EXT_EGRESS) C.dir_of[C.D++] = 0;
    if (dirs & CLS_EXT_INGRESS) C.dir_of[C.D++] = 1;
    ext_classes(e, sp, C);
    if (C.lo.size() > (1u << 30)) return fail(e, CLS_E_INVAL, "reach external above 2^30 classes (K %zu)", C.lo.size());
    C.K = uint32_t(C.lo.size());
    C.lines = uint64_t(C.D) * R.P * R.N;              // <= 2^35
    if (C.lines > kReachMaxCells / C.K)
        return fail(e, CLS_E_INVAL, "reach external above 2^36 rows (K %u classes x N %u endpoints x %u probes x %u "
                                    "directions)", C.K, R.N, R.P, C.D);
    R.cells = C.lines * C.K;
    // whole lines per tile (one when K exceeds reach_tile): no range crosses a tile
    C.per_tile = std::max<uint64_t>(1, e->opts.reach_tile / C.K);
    R.tile = C.per_tile * C.K;                        // <= max(reach_tile, K) <= 2^30
    R.mode = flags & (CLS_F_CONN_CLS | CLS_F_FORCE_LINEAR);
    R.s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    C.o = *o;
    C.cap = o->ranges ? std::min(o->cap, R.cells) : 0;
    R.off_addr = (size_t(R.N) * 4 + 15) & ~size_t(15);
    R.off_probe = (R.off_addr + size_t(R.N) * (R.k16 ? 16 : 4) + 15) & ~size_t(15);
    C.off_lo = (R.off_probe + size_t(R.P) * sizeof(uint2) + 15) & ~size_t(15);
    R.tab_bytes = C.off_lo + ((size_t(C.K) * 4 + 15) & ~size_t(15));
    if (o->n_classes) *o->n_classes = C.K;
    return CLS_OK;
}

// The endpoint and probe tables with the class starts behind them.
static int ext_upload(cls_engine* e, const cls_reach_spec* sp, const ExtCall& C) {
    const ReachCall& R = C.R;
    std::vector<uint8_t> tab(R.tab_bytes, 0);
    std::memcpy(tab.data(), sp->if_id, size_t(R.N) * 4);
    std::memcpy(tab.data() + R.off_addr, R.k16 ? static_cast<const void*>(sp->addr16) : sp->addr4,
                size_t(R.N) * (R.k16 ? 16 : 4));
    uint2* pr = reinterpret_cast<uint2*>(tab.data() + R.off_probe);
    for (uint32_t p = 0; p < R.P; ++p) pr[p] = uint2{uint32_t(sp->sport[p]) | uint32_t(sp->dport[p]) << 16, sp->proto[p]};
    std::memcpy(tab.data() + C.off_lo, C.lo.data(), size_t(C.K) * 4);
    return reach_upload_tab(e, R, tab);
}

// Where the per-line sums and the histogram accumulate: the caller's device
// memory, or the engine's for a host call.
static uint32_t* ext_runs(cls_engine* e, const ExtCall& C) {
    return !C.o.runs_out ? nullptr : C.R.dev ? C.o.runs_out : e->r_runs.as<uint32_t>();
}
static unsigned long long* ext_allow(cls_engine* e, const ExtCall& C) {
    return !C.o.allow_addrs_out ? nullptr
           : C.R.dev            ? reinterpret_cast<unsigned long long*>(C.o.allow_addrs_out)
                                : e->r_pallow.as<unsigned long long>();
}
static unsigned long long* ext_hist(cls_engine* e, const ExtCall& C) {
    return !C.o.hist_out ? nullptr
           : C.R.dev     ? reinterpret_cast<unsigned long long*>(C.o.hist_out)
                         : e->r_phist.as<unsigned long long>();
}

// Beyond reach_scratch: a host call's records (cap of them) and sums, the
// tile's chunk counts and first indices, the running total; all cleared.
static int ext_scratch(cls_engine* e, const ExtCall& C) {
    const ReachCall& R = C.R;
    const size_t n = size_t(std::min(R.tile, R.cells)), hb = size_t(C.D) * R.P * 4 * 8;
    if (!R.dev) {
        if (C.o.ranges) HIPC(e, reach_grow(e, e->r_changes, size_t(C.cap) * sizeof(cls_addr_range)));
        if (C.o.runs_out) HIPC(e, reach_grow(e, e->r_runs, size_t(C.lines) * 4));
        if (C.o.allow_addrs_out) HIPC(e, reach_grow(e, e->r_pallow, size_t(C.lines) * 8));
        if (C.o.hist_out) HIPC(e, reach_grow(e, e->r_phist, hb));
    }
    if (C.scan()) {
        const size_t chunks = (n + kReachChunk - 1) / kReachChunk;
        HIPC(e, reach_grow(e, e->r_dcount, chunks * 4));
        HIPC(e, reach_grow(e, e->r_dbase, chunks * 8));
        HIPC(e, reach_grow(e, e->r_dtotal, 8));
        HIPC(e, hipMemsetAsync(e->r_dtotal.p, 0, 8, R.s));
    }
    if (uint32_t* p = ext_runs(e, C)) HIPC(e, hipMemsetAsync(p, 0, size_t(C.lines) * 4, R.s));
    if (unsigned long long* p = ext_allow(e, C)) HIPC(e, hipMemsetAsync(p, 0, size_t(C.lines) * 8, R.s));
    if (unsigned long long* p = ext_hist(e, C)) HIPC(e, hipMemsetAsync(p, 0, hb, R.s));
    return CLS_OK;
}

// One tile: the nl whole lines from `line` on.
static int ext_tile(cls_engine* e, const ExtCall& C, uint64_t line, uint32_t nl) {
    const ReachCall& R = C.R;
    const uint8_t* tab = e->r_tab.as<uint8_t>();
    const uint32_t n = nl * C.K;
    const uint64_t q = line / R.N;                    // the first line's (dir, probe)
    const ReachExtTile T{R.N, R.P, uint32_t(q / R.P), uint32_t(q % R.P), uint32_t(line % R.N), C.K, n,
                         {C.dir_of[0], C.dir_of[1]}, reinterpret_cast<const uint32_t*>(tab + C.off_lo)};
    ReachExtExpand X{};
    X.ep_if = reinterpret_cast<const uint32_t*>(tab);
    X.ep_addr = tab + R.off_addr;
    X.probe = reinterpret_cast<const uint2*>(tab + R.off_probe);
    X.ext_if = C.ext_if;
    X.src_if = e->r_sif.as<uint32_t>(); X.dst_if = e->r_dif.as<uint32_t>();
    X.src = e->r_src.p; X.dst = e->r_dst.p;
    X.sport = e->r_sport.as<uint16_t>(); X.dport = e->r_dport.as<uint16_t>();
    X.proto = e->r_proto.as<uint8_t>();
    HIPC(e, launch_reach_ext_expand(T, X, R.k16, e->n_cu, R.s));
    // the evaluator, unchanged: a device batch over the expanded arrays
    cls_conn_soa c{};
    c.pkt.af = R.k16 ? CLS_AF_V16 : CLS_AF_V4;
    if (R.k16) {
        c.pkt.src16 = e->r_src.as<uint8_t>(); c.pkt.dst16 = e->r_dst.as<uint8_t>();
    } else {
        c.pkt.src4 = e->r_src.as<uint32_t>(); c.pkt.dst4 = e->r_dst.as<uint32_t>();
    }
    c.pkt.sport = X.sport; c.pkt.dport = X.dport; c.pkt.proto = X.proto;
    c.src_if = X.src_if; c.dst_if = X.dst_if;
    const uint8_t* v = e->r_verdict.as<uint8_t>();
    const int rc = connect_locked(e, &c, n, e->r_verdict.as<uint8_t>(), CLS_F_DEVICE | R.mode, R.s, false);
    if (rc != CLS_OK) return rc;
    uint32_t* runs = ext_runs(e, C);
    unsigned long long* allow = ext_allow(e, C);
    unsigned long long* hist = ext_hist(e, C);
    uint32_t* count = C.scan() ? e->r_dcount.as<uint32_t>() : nullptr;
    HIPC(e, launch_reach_ext_count(T, v, count, runs ? runs + line : nullptr, allow ? allow + line : nullptr,
                                   hist ? hist + 4 * q : nullptr, e->n_cu, R.s));
    if (!C.scan()) return CLS_OK;
    unsigned long long* at = e->r_dbase.as<unsigned long long>();
    HIPC(e, launch_reach_diff_scan((n + kReachChunk - 1) / kReachChunk, count, at,
                                   e->r_dtotal.as<unsigned long long>(), R.s));
    cls_addr_range* rec = !C.o.ranges ? nullptr : R.dev ? C.o.ranges : e->r_changes.as<cls_addr_range>();
    HIPC(e, launch_reach_ext_emit(T, v, at, reinterpret_cast<uint4*>(rec), C.cap, e->n_cu, R.s));
    return CLS_OK;
}

// A host call's sums, total and records through the engine's buffers (it
// waits for the total and copies that many records, none past them); a device
// call's total.  A device call is stream-ordered (conn_last).
static int ext_outputs(cls_engine* e, const ExtCall& C) {
    const ReachCall& R = C.R;
    if (R.dev) {
        if (C.o.n_ranges) HIPC(e, hipMemcpyAsync(C.o.n_ranges, e->r_dtotal.p, 8, hipMemcpyDeviceToDevice, R.s));
        e->conn_last = R.s;
        return CLS_OK;
    }
    const hipMemcpyKind kind = hipMemcpyDeviceToHost;
    if (C.o.runs_out) HIPC(e, hipMemcpyAsync(C.o.runs_out, e->r_runs.p, size_t(C.lines) * 4, kind, R.s));
    if (C.o.allow_addrs_out) HIPC(e, hipMemcpyAsync(C.o.allow_addrs_out, e->r_pallow.p, size_t(C.lines) * 8, kind, R.s));
    if (C.o.hist_out) HIPC(e, hipMemcpyAsync(C.o.hist_out, e->r_phist.p, size_t(C.D) * R.P * 4 * 8, kind, R.s));
    uint64_t total = 0;
    if (C.o.n_ranges) HIPC(e, hipMemcpyAsync(&total, e->r_dtotal.p, 8, kind, R.s));
    HIPC(e, hipStreamSynchronize(R.s));
    const uint64_t n = std::min(total, C.cap);
    if (C.o.ranges && n) {
        HIPC(e, hipMemcpyAsync(C.o.ranges, e->r_changes.p, size_t(n) * sizeof(cls_addr_range), kind, R.s));
        HIPC(e, hipStreamSynchronize(R.s));
    }
    if (C.o.n_ranges) *C.o.n_ranges = total;
    e->conn_last = nullptr;
    return CLS_OK;
}

extern "C" int cls_reach_external(cls_engine* e, const cls_reach_spec* spec, uint32_t ext_if, uint32_t dirs,
                                  const cls_reach_ext_out* out, uint32_t flags, void* stream) {
    if (!e || !spec) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    if (!out) return fail(e, CLS_E_INVAL, "reach external without outputs");
    ExtCall C;
    int rc = ext_inputs(e, spec, ext_if, dirs, out, flags, stream, C);
    if (rc != CLS_OK) return rc;
    rc = ext_upload(e, spec, C);
    if (rc == CLS_OK) rc = reach_scratch(e, C.R);
    if (rc == CLS_OK) rc = ext_scratch(e, C);
    for (uint64_t line = 0; rc == CLS_OK && line < C.lines; line += C.per_tile)
        rc = ext_tile(e, C, line, uint32_t(std::min(C.per_tile, C.lines - line)));
    if (rc == CLS_OK) rc = ext_outputs(e, C);
    return rc;
}

// ---- cls_reach_hops: multi-hop closure and blast radius of the matrix -----
// The graph: an edge s -> d (s != d) where some probe's cell is
// CLS_CONN_ALLOW.  Per tile the fold launch (k_reach_hops.hip) ORs the tile's
// ALLOW cells into the adjacency bitmap r_adj -- behind the evaluator in
// reach_tile, or alone over a caller's matrix -- and one launch at the end runs
// the breadth-first search from every source and writes every output.

struct HopsCall {
    ReachCall R;
    const uint8_t* matrix = nullptr;       // null: the matrix of the spec is evaluated
    uint32_t H = 0, W = 0, rows = 0;       // levels (1 .. 254); words per bit row; source rows per workgroup
    cls_reach_hops_out o{};
};

// Checks everything a refusal can depend on: no device work is queued before
// this returns CLS_OK.
static int hops_inputs(cls_engine* e, const cls_reach_spec* sp, const uint8_t* matrix, uint32_t max_hops,
                       const cls_reach_hops_out* o, uint32_t flags, void* stream, HopsCall& C) {
    ReachCall& R = C.R;
    if (matrix) {
        if (!sp->n_endpoints || !sp->n_probes) return fail(e, CLS_E_INVAL, "reach hops without endpoints or probes");
        if (flags & (CLS_F_COUNT | CLS_F_CONN_CLS | CLS_F_FORCE_LINEAR))
            return fail(e, CLS_E_INVAL, "reach hops over a matrix evaluates nothing: no CLS_F_COUNT, CLS_F_CONN_CLS "
                                        "or CLS_F_FORCE_LINEAR");
    } else {
        const int rc = reach_spec(e, sp, R);
        if (rc != CLS_OK) return rc;
        if (!sp->dport) return fail(e, CLS_E_INVAL, "missing reach matrix arrays");
    }
    if (flags & CLS_F_NO_VERDICT) return fail(e, CLS_E_INVAL, "reach hops: no CLS_F_NO_VERDICT");
    if (!o->hops_out && !o->reach_out && !o->exposed_out && !o->level_out && !o->closure_out)
        return fail(e, CLS_E_INVAL, "reach hops without hops_out, reach_out, exposed_out, level_out or closure_out");
    if (max_hops > 254) return fail(e, CLS_E_INVAL, "reach hops: max_hops %u above 254", max_hops);
    int rc = reach_cells(e, sp, R);
    if (rc != CLS_OK) return rc;
    if (R.N > 32768) return fail(e, CLS_E_INVAL, "reach hops above 32768 endpoints (N %u)", R.N);
    R.dev = flags & CLS_F_DEVICE;
    if (R.dev && (!aligned(matrix, 16) || !aligned(o->hops_out, 16) || !aligned(o->level_out, 8) ||
                  !aligned(o->closure_out, 8) || !aligned(o->reach_out, 4) || !aligned(o->exposed_out, 4)))
        return fail(e, CLS_E_INVAL, "device reach hops: matrix, hops_out 16-byte, level_out, closure_out 8-byte, "
                                    "reach_out, exposed_out 4-byte aligned");
    if (!matrix) {
        rc = reach_spec_ifs(e, sp);
        if (rc != CLS_OK) return rc;
    }
    reach_resolve(e, flags, stream, R);
    C.matrix = matrix;
    C.H = max_hops ? max_hops : 254;
    C.W = (R.N + 63) / 64;
    C.rows = reach_hops_rows(R.N, e->opts.hops_rows);
    C.o = *o;
    return CLS_OK;
}

// Where the launch writes: the caller's device memory, or the engine's for a
// host call.
static uint8_t* hops_hops(cls_engine* e, const HopsCall& C) {
    return !C.o.hops_out ? nullptr : C.R.dev ? C.o.hops_out : e->r_hhops.as<uint8_t>();
}
static uint32_t* hops_reach(cls_engine* e, const HopsCall& C) {
    return !C.o.reach_out ? nullptr : C.R.dev ? C.o.reach_out : e->r_hreach.as<uint32_t>();
}
static uint32_t* hops_exposed(cls_engine* e, const HopsCall& C) {
    return !C.o.exposed_out ? nullptr : C.R.dev ? C.o.exposed_out : e->r_hexposed.as<uint32_t>();
}
static unsigned long long* hops_levels(cls_engine* e, const HopsCall& C) {
    return !C.o.level_out ? nullptr
           : C.R.dev      ? reinterpret_cast<unsigned long long*>(C.o.level_out)
                          : e->r_hlevel.as<unsigned long long>();
}
static unsigned long long* hops_closure(cls_engine* e, const HopsCall& C) {
    return !C.o.closure_out ? nullptr
           : C.R.dev        ? reinterpret_cast<unsigned long long*>(C.o.closure_out)
                            : e->r_hclosure.as<unsigned long long>();
}

// The bitmap (cleared), a host matrix's tile, a host call's outputs; the
// accumulators cleared.  The evaluating form's tile arrays: reach_scratch.
static int hops_scratch(cls_engine* e, const HopsCall& C) {
    const ReachCall& R = C.R;
    const size_t bits = size_t(R.N) * C.W * 8;
    HIPC(e, reach_grow(e, e->r_adj, bits));
    HIPC(e, hipMemsetAsync(e->r_adj.p, 0, bits, R.s));
    if (C.matrix && !R.dev) HIPC(e, reach_grow(e, e->r_base, size_t(std::min(R.tile, R.cells))));
    if (!R.dev) {
        if (C.o.hops_out) HIPC(e, reach_grow(e, e->r_hhops, size_t(R.N) * R.N));
        if (C.o.reach_out) HIPC(e, reach_grow(e, e->r_hreach, size_t(R.N) * 4));
        if (C.o.exposed_out) HIPC(e, reach_grow(e, e->r_hexposed, size_t(R.N) * 4));
        if (C.o.level_out) HIPC(e, reach_grow(e, e->r_hlevel, 256 * 8));
        if (C.o.closure_out) HIPC(e, reach_grow(e, e->r_hclosure, bits));
    }
    if (uint32_t* p = hops_exposed(e, C)) HIPC(e, hipMemsetAsync(p, 0, size_t(R.N) * 4, R.s));
    if (unsigned long long* p = hops_levels(e, C)) HIPC(e, hipMemsetAsync(p, 0, 256 * 8, R.s));
    return CLS_OK;
}

// One tile of a caller's matrix: cells [first, first + n), a host matrix's
// through the scratch.
static int hops_fold_tile(cls_engine* e, const HopsCall& C, uint64_t first, uint32_t n) {
    const ReachCall& R = C.R;
    const uint64_t row = first / R.N;
    const ReachTile T{R.N, uint32_t(row / R.N), uint32_t(row % R.N), uint32_t(first % R.N), n};
    const uint8_t* v = C.matrix + first;
    if (!R.dev) {
        HIPC(e, hipMemcpyAsync(e->r_base.p, v, n, hipMemcpyHostToDevice, R.s));
        v = e->r_base.as<uint8_t>();
    }
    HIPC(e, launch_reach_adj_fold(T, v, R.adj, e->n_cu, R.s));
    return CLS_OK;
}

// The search, and a host call's results through the engine's buffers; a
// device call is stream-ordered (conn_last).
static int hops_outputs(cls_engine* e, const HopsCall& C) {
    const ReachCall& R = C.R;
    HIPC(e, launch_reach_hops_bfs(R.N, C.H, C.rows, R.adj, hops_hops(e, C), hops_reach(e, C), hops_exposed(e, C),
                                  hops_levels(e, C), hops_closure(e, C), R.s));
    if (R.dev) {
        e->conn_last = R.s;
        return CLS_OK;
    }
    const hipMemcpyKind kind = hipMemcpyDeviceToHost;
    if (C.o.hops_out) HIPC(e, hipMemcpyAsync(C.o.hops_out, e->r_hhops.p, size_t(R.N) * R.N, kind, R.s));
    if (C.o.reach_out) HIPC(e, hipMemcpyAsync(C.o.reach_out, e->r_hreach.p, size_t(R.N) * 4, kind, R.s));
    if (C.o.exposed_out) HIPC(e, hipMemcpyAsync(C.o.exposed_out, e->r_hexposed.p, size_t(R.N) * 4, kind, R.s));
    if (C.o.level_out) HIPC(e, hipMemcpyAsync(C.o.level_out, e->r_hlevel.p, 256 * 8, kind, R.s));
    if (C.o.closure_out) HIPC(e, hipMemcpyAsync(C.o.closure_out, e->r_hclosure.p, size_t(R.N) * C.W * 8, kind, R.s));
    HIPC(e, hipStreamSynchronize(R.s));
    e->conn_last = nullptr;
    return CLS_OK;
}

extern "C" int cls_reach_hops(cls_engine* e, const cls_reach_spec* spec, const uint8_t* matrix, uint32_t max_hops,
                              const cls_reach_hops_out* out, uint32_t flags, void* stream) {
    if (!e || !spec) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    if (!out) return fail(e, CLS_E_INVAL, "reach hops without outputs");
    HopsCall C;
    ReachCall& R = C.R;
    int rc = hops_inputs(e, spec, matrix, max_hops, out, flags, stream, C);
    if (rc != CLS_OK) return rc;
    rc = matrix ? reach_follow(e, R) : reach_upload(e, spec, R);
    if (rc == CLS_OK && !matrix) rc = reach_scratch(e, R);
    if (rc == CLS_OK) rc = hops_scratch(e, C);
    R.adj = e->r_adj.as<unsigned long long>();
    for (uint64_t first = 0; rc == CLS_OK && first < R.cells; first += R.tile) {
        const uint32_t n = uint32_t(std::min(R.tile, R.cells - first));
        rc = matrix ? hops_fold_tile(e, C, first, n) : reach_tile(e, R, first, n);
    }
    if (rc == CLS_OK) rc = hops_outputs(e, C);
    return rc;
}

// ---- cls_reach_classes: equivalent endpoints and their quotient matrix ----
// Rounds of two passes over the matrix (k_reach_classes.hip) around the host
// grouping (reach_classes.cpp): the fold pass -- behind the evaluator in
// reach_tile, or alone over a matrix in memory -- then class_group, then the
// verify pass over the candidate.  A pass streams the caller's device matrix
// or device verdict_out where there is one, a host matrix tile by tile
// through r_base, and evaluates again otherwise.  The call waits for every
// pass: the candidate decides the verify table's size, the verify pass's
// flag whether another round follows.

struct ClassesCall {
    ReachCall R;
    const uint8_t* matrix = nullptr;       // null: the matrix of the spec is evaluated
    bool evaluated = false;                // the evaluating form's first pass has run
    cls_reach_classes_out o{};
};

// Checks everything a refusal can depend on: no device work is queued before
// this returns CLS_OK.
static int classes_inputs(cls_engine* e, const cls_reach_spec* sp, const uint8_t* matrix,
                          const cls_reach_classes_out* o, uint32_t flags, void* stream, ClassesCall& C) {
    ReachCall& R = C.R;
    if (matrix) {
        if (!sp->n_endpoints || !sp->n_probes)
            return fail(e, CLS_E_INVAL, "reach classes without endpoints or probes");
        if (flags & (CLS_F_CONN_CLS | CLS_F_FORCE_LINEAR))
            return fail(e, CLS_E_INVAL, "reach classes over a matrix evaluates nothing: no CLS_F_CONN_CLS or "
                                        "CLS_F_FORCE_LINEAR");
    } else {
        const int rc = reach_spec(e, sp, R);
        if (rc != CLS_OK) return rc;
        if (!sp->dport) return fail(e, CLS_E_INVAL, "missing reach matrix arrays");
    }
    if (flags & (CLS_F_COUNT | CLS_F_NO_VERDICT))
        return fail(e, CLS_E_INVAL, "reach classes: no CLS_F_COUNT, no CLS_F_NO_VERDICT");
    if (const char* why = class_refuse(sp->n_endpoints, o)) return fail(e, CLS_E_INVAL, "%s (N %u)", why, sp->n_endpoints);
    int rc = reach_cells(e, sp, R);
    if (rc != CLS_OK) return rc;
    R.dev = flags & CLS_F_DEVICE;
    if (R.dev && (!aligned(matrix, 16) || !aligned(o->verdict_out, 16) || !aligned(o->class_out, 4) ||
                  !aligned(o->rep_out, 4) || !aligned(o->size_out, 4)))
        return fail(e, CLS_E_INVAL, "device reach classes: matrix, verdict_out 16-byte, class_out, rep_out, "
                                    "size_out 4-byte aligned");
    if (!matrix) {
        rc = reach_spec_ifs(e, sp);
        if (rc != CLS_OK) return rc;
    }
    reach_resolve(e, flags, stream, R);
    C.matrix = matrix;
    C.o = *o;
    if (!matrix) R.verdict_out = o->verdict_out;
    return CLS_OK;
}

// A scratch buffer of the call; what cannot be allocated is CLS_E_NOMEM.
static int classes_grow(cls_engine* e, DevBuf& d, size_t bytes) {
    const hipError_t h = reach_grow(e, d, bytes);
    if (h == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return fail(e, CLS_E_NOMEM, "reach classes: %zu bytes of device scratch", bytes);
    }
    HIPC(e, h);
    return CLS_OK;
}

// One pass (R.cpass) over every tile of the matrix.
static int classes_pass(cls_engine* e, ClassesCall& C) {
    ReachCall& R = C.R;
    // the matrix in device memory, where there is one
    const uint8_t* devmat = !R.dev ? nullptr : C.matrix ? C.matrix : C.evaluated ? C.o.verdict_out : nullptr;
    // (a host verdict_out is copied out by the first evaluation only)
    R.verdict_out = C.matrix || (C.evaluated && !R.dev) ? nullptr : C.o.verdict_out;
    for (uint64_t first = 0; first < R.cells; first += R.tile) {
        const uint32_t n = uint32_t(std::min(R.tile, R.cells - first));
        if (!devmat && !C.matrix) {
            const int rc = reach_tile(e, R, first, n);
            if (rc != CLS_OK) return rc;
            continue;
        }
        const uint64_t row = first / R.N;
        const ReachTile T{R.N, uint32_t(row / R.N), uint32_t(row % R.N), uint32_t(first % R.N), n};
        const uint8_t* v = devmat ? devmat + first : e->r_base.as<uint8_t>();
        if (!devmat) HIPC(e, hipMemcpyAsync(e->r_base.p, C.matrix + first, n, hipMemcpyHostToDevice, R.s));
        HIPC(e, class_launch(*R.cpass, T, v, R.s));
    }
    if (!C.matrix) C.evaluated = true;
    return CLS_OK;
}

// The rounds; on CLS_OK cand holds the verified classes, numbered canonically,
// and the verify table is in r_ctab.
static int classes_rounds(cls_engine* e, ClassesCall& C, std::vector<uint32_t>& cand, ClassFold& f, uint32_t& n_classes,
                          uint32_t& rounds) {
    ReachCall& R = C.R;
    const size_t pn = size_t(R.P) * R.N;
    int rc = classes_grow(e, e->r_csums, pn * 16);
    if (rc == CLS_OK) rc = classes_grow(e, e->r_cdiag, pn);
    if (rc == CLS_OK) rc = classes_grow(e, e->r_cmask, 64);
    if (rc == CLS_OK) rc = classes_grow(e, e->r_ccls, size_t(R.N) * 4);
    if (rc == CLS_OK && C.matrix && !R.dev) rc = classes_grow(e, e->r_base, size_t(std::min(R.tile, R.cells)));
    if (rc != CLS_OK) return rc;
    ClassKeys keys;
    f.sums.resize(pn * 2);
    f.diag.resize(pn);
    uint32_t* mask = e->r_cmask.as<uint32_t>();           // 8 words, then the verify pass's flag
    ClassPass ps;
    R.cpass = &ps;
    for (uint32_t round = 0; round < kClassRounds; ++round) {
        ps = ClassPass{};
        ps.seed_r = class_seed(round, 0);
        ps.seed_c = class_seed(round, 1);
        ps.sums = e->r_csums.as<unsigned long long>();
        ps.diag = e->r_cdiag.as<uint8_t>();
        ps.mask = mask;
        HIPC(e, hipMemsetAsync(e->r_csums.p, 0, pn * 16, R.s));
        HIPC(e, hipMemsetAsync(e->r_cmask.p, 0, 64, R.s));
        rc = classes_pass(e, C);
        if (rc != CLS_OK) return rc;
        HIPC(e, hipMemcpyAsync(f.sums.data(), e->r_csums.p, pn * 16, hipMemcpyDeviceToHost, R.s));
        HIPC(e, hipMemcpyAsync(f.diag.data(), e->r_cdiag.p, pn, hipMemcpyDeviceToHost, R.s));
        HIPC(e, hipMemcpyAsync(f.mask, e->r_cmask.p, 32, hipMemcpyDeviceToHost, R.s));
        HIPC(e, hipStreamSynchronize(R.s));
        n_classes = class_group(R.N, R.P, e->opts.classes_key_bits, round, f, keys, cand);
        const size_t tb = class_table_words(R.P, n_classes) * 4;
        rc = classes_grow(e, e->r_ctab, tb);
        if (rc != CLS_OK) return rc;
        HIPC(e, hipMemsetAsync(e->r_ctab.p, 0, tb, R.s));
        HIPC(e, hipMemcpyAsync(e->r_ccls.p, cand.data(), size_t(R.N) * 4, hipMemcpyHostToDevice, R.s));
        ps = ClassPass{};
        ps.verify = true;
        ps.cls = e->r_ccls.as<uint32_t>();
        ps.C = n_classes;
        ps.tab = e->r_ctab.as<uint32_t>();
        ps.bad = mask + 8;
        rc = classes_pass(e, C);
        if (rc != CLS_OK) return rc;
        uint32_t bad = 0;
        HIPC(e, hipMemcpyAsync(&bad, mask + 8, 4, hipMemcpyDeviceToHost, R.s));
        HIPC(e, hipStreamSynchronize(R.s));
        rounds = round + 1;
        if (!bad) return CLS_OK;
    }
    return fail(e, CLS_E_INVAL, "reach classes: did not converge in %u rounds (classes_key_bits %u)", kClassRounds,
                e->opts.classes_key_bits);
}

// The results to the caller's outputs, device or host.
static int classes_outputs(cls_engine* e, ClassesCall& C, const std::vector<uint32_t>& cand, const ClassFold& f,
                           uint32_t n_classes, uint32_t rounds) {
    const ReachCall& R = C.R;
    const cls_reach_classes_out& o = C.o;
    // (a host call's outputs: plain copies)
    auto put = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        if (!dst || !bytes) return hipSuccess;
        if (R.dev) return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, R.s);
        std::memcpy(dst, src, bytes);
        return hipSuccess;
    };
    ClassResult r;
    const bool per_class = (o.rep_out || o.size_out || o.self_out || o.quot_out) && n_classes <= o.class_cap;
    if (per_class) {
        std::vector<uint32_t> tab(class_table_words(R.P, n_classes));
        HIPC(e, hipMemcpyAsync(tab.data(), e->r_ctab.p, tab.size() * 4, hipMemcpyDeviceToHost, R.s));
        HIPC(e, hipStreamSynchronize(R.s));
        class_result(R.N, R.P, n_classes, cand.data(), tab.data(), r);
        HIPC(e, put(o.rep_out, r.rep.data(), size_t(n_classes) * 4));
        HIPC(e, put(o.size_out, r.size.data(), size_t(n_classes) * 4));
        HIPC(e, put(o.self_out, r.self.data(), r.self.size()));
        HIPC(e, put(o.quot_out, r.quot.data(), r.quot.size()));
    }
    HIPC(e, put(o.class_out, cand.data(), size_t(R.N) * 4));
    if (C.matrix && o.verdict_out && o.verdict_out != C.matrix) {
        if (R.dev) HIPC(e, hipMemcpyAsync(o.verdict_out, C.matrix, size_t(R.cells), hipMemcpyDeviceToDevice, R.s));
        else std::memmove(o.verdict_out, C.matrix, size_t(R.cells));
    }
    HIPC(e, hipStreamSynchronize(R.s));
    e->conn_last = nullptr;
    if (o.n_classes) *o.n_classes = n_classes;
    if (o.rounds) *o.rounds = rounds;
    if (o.sums_out) std::memcpy(o.sums_out, f.sums.data(), f.sums.size() * 8);
    return CLS_OK;
}

extern "C" int cls_reach_classes(cls_engine* e, const cls_reach_spec* spec, const uint8_t* matrix,
                                 const cls_reach_classes_out* out, uint32_t flags, void* stream) {
    if (!e || !spec) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    ClassesCall C;
    ReachCall& R = C.R;
    int rc = classes_inputs(e, spec, matrix, out, flags, stream, C);
    if (rc != CLS_OK) return rc;
    rc = matrix ? reach_follow(e, R) : reach_upload(e, spec, R);
    if (rc == CLS_OK && !matrix) rc = reach_scratch(e, R);
    if (rc != CLS_OK) return rc;
    try {
        std::vector<uint32_t> cand;
        ClassFold f;
        uint32_t n_classes = 0, rounds = 0;
        rc = classes_rounds(e, C, cand, f, n_classes, rounds);
        if (rc == CLS_OK) rc = classes_outputs(e, C, cand, f, n_classes, rounds);
    } catch (const std::bad_alloc&) {
        rc = fail(e, CLS_E_NOMEM, "reach classes: out of host memory");
    }
    // (whatever was enqueued has run, or its stream failed: nothing stream-ordered is left behind)
    if (rc != CLS_OK && rc != CLS_E_INVAL) (void)hipStreamSynchronize(R.s);
    return rc;
}
