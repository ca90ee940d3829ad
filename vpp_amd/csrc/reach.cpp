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
// and its own outputs at the end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/contivcls.h"
#include "engine_int.hpp"
#include "kernels.hpp"

using namespace cls;

constexpr uint64_t kReachMaxCells = 1ull << 36;   // P x N x N of one call

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

// Checks everything a refusal can depend on: no device work is queued before
// this returns CLS_OK.
static int reach_inputs(cls_engine* e, const cls_reach_spec* sp, uint8_t* verdict_out, uint64_t* hist_out,
                        uint32_t* allow_out, uint32_t flags, void* stream, ReachCall& R) {
    R.k16 = sp->af == CLS_AF_V16;
    if (!R.k16 && sp->af != CLS_AF_V4) return fail(e, CLS_E_INVAL, "af must be CLS_AF_V4 or CLS_AF_V16");
    if (!sp->n_endpoints || !sp->n_probes) return fail(e, CLS_E_INVAL, "reach matrix without endpoints or probes");
    if (!sp->if_id || !(R.k16 ? static_cast<const void*>(sp->addr16) : sp->addr4) || !sp->proto || !sp->sport ||
        !sp->dport)
        return fail(e, CLS_E_INVAL, "missing reach matrix arrays");
    // (a diff has outputs of its own, and its verdict_out may simply be NULL)
    if (!R.base && !verdict_out && !hist_out && !allow_out)
        return fail(e, CLS_E_INVAL, "reach matrix without an output");
    if (!R.base && !verdict_out && !(flags & CLS_F_NO_VERDICT))
        return fail(e, CLS_E_INVAL, "verdict_out is NULL without CLS_F_NO_VERDICT");
    R.N = sp->n_endpoints;
    R.P = sp->n_probes;
    // (N^2 first: P x N^2 <= 2^36 with P >= 1 needs N <= 2^18)
    if (R.N > (1u << 18) || uint64_t(R.N) * R.N > kReachMaxCells / R.P)
        return fail(e, CLS_E_INVAL, "reach matrix above 2^36 cells");
    R.cells = uint64_t(R.N) * R.N * R.P;
    R.dev = flags & CLS_F_DEVICE;
    if (R.dev && (!aligned(verdict_out, 16) || !aligned(hist_out, 8) || !aligned(allow_out, 4)))
        return fail(e, CLS_E_INVAL, "device outputs: verdict_out 16-byte, hist_out 8-byte, allow_out 4-byte aligned");
    const uint32_t n_ifs = uint32_t(e->if_acl.size());
    for (uint32_t i = 0; i < R.N; ++i)
        if (sp->if_id[i] >= n_ifs) return fail(e, CLS_E_INVAL, "endpoint %u: unknown interface id", i);
    R.mode = flags & (CLS_F_COUNT | CLS_F_CONN_CLS | CLS_F_FORCE_LINEAR);
    R.tile = e->opts.reach_tile;
    R.s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    R.verdict_out = verdict_out;
    R.hist_out = hist_out;
    R.allow_out = allow_out;
    R.off_addr = (size_t(R.N) * 4 + 15) & ~size_t(15);
    R.off_probe = R.off_addr + size_t(R.N) * (R.k16 ? 16 : 4);
    R.off_probe = (R.off_probe + 15) & ~size_t(15);
    R.tab_bytes = R.off_probe + size_t(R.P) * sizeof(uint2);
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

// The endpoint and probe tables, uploaded once per call from the engine's
// copy (the caller's arrays are not read after this); nothing is copied when
// the last call's tables are the same.  Orders the call behind the last
// stream-ordered batch of another stream, which may still use the scratch.
static int reach_upload(cls_engine* e, const cls_reach_spec* sp, const ReachCall& R) {
    HIPC(e, hipSetDevice(e->device));
    if (e->conn_last && e->conn_last != R.s) {
        if (!e->conn_sync_ev) HIPC(e, hipEventCreateWithFlags(&e->conn_sync_ev, hipEventDisableTiming));
        HIPC(e, hipEventRecord(e->conn_sync_ev, e->conn_last));
        HIPC(e, hipStreamWaitEvent(R.s, e->conn_sync_ev, 0));
    }
    std::vector<uint8_t> tab(R.tab_bytes, 0);
    std::memcpy(tab.data(), sp->if_id, size_t(R.N) * 4);
    std::memcpy(tab.data() + R.off_addr, R.k16 ? static_cast<const void*>(sp->addr16) : sp->addr4,
                size_t(R.N) * (R.k16 ? 16 : 4));
    uint2* pr = reinterpret_cast<uint2*>(tab.data() + R.off_probe);
    for (uint32_t p = 0; p < R.P; ++p) pr[p] = uint2{uint32_t(sp->sport[p]) | uint32_t(sp->dport[p]) << 16, sp->proto[p]};
    const void* was = e->r_tab.p;
    HIPC(e, reach_grow(e, e->r_tab, R.tab_bytes));
    if (e->r_tab.p == was && e->reach_up == tab) return CLS_OK;
    const int rc = conn_quiesce(e);                  // an earlier copy may still read reach_up
    if (rc != CLS_OK) return rc;
    e->reach_up.swap(tab);
    HIPC(e, hipMemcpyAsync(e->r_tab.p, e->reach_up.data(), R.tab_bytes, hipMemcpyHostToDevice, R.s));
    return CLS_OK;
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
