// Connection batches (cls_connect_batch, cls_connect_rules): the host side of
// the connection path -- the bitmap form of linear ACLs, the pair launches'
// images, and connect_locked as a sequence of stages: the batch's inputs, the
// plan over the bindings (ConnPlan), the large ACLs' classify launches, the
// upload of the call's tables, the LDS plan, the launch with its counter
// flush, the copy back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/contivcls.h"
#include "compile.hpp"
#include "engine_int.hpp"
#include "kernels.hpp"

using namespace cls;

constexpr uint64_t kConnClsMinBatch = 1ull << 16;  // connection batches that use the classifier images
constexpr uint32_t kConnClsMinRules = 64;          // ACLs evaluated by the classifier in connection batches
constexpr uint32_t kConnClsWork = 2048;            // ... when touches x rules >= this x batch size (host batch)
constexpr uint32_t kConnClsDevRules = 2048;        // ... when it has this many rules (device batch)
constexpr uint32_t kConnBmMinRules = 8;            // linear IPv4 ACLs given the bitmap form (conn_bitmap4) ...
constexpr size_t kConnBmMaxWords = 12288;          // ... when their tables take at most 48 KiB

// The bitmap form of a linear IPv4 ACL (kernels.hpp kConnBmHeader): for the
// source, the destination and each protocol's destination port, the
// elementary intervals of the rules' prefixes (port ranges) and, per
// interval, the bit row of the rules whose term holds there -- each
// predicate evaluated exactly as the scan does (conn_match, the meta TERM bit,
// port_in) at the interval's first value, which is exact because prefixes
// and ranges only change membership at the interval starts.  Appends the
// words (16-B multiple) to `out`; false (nothing appended) when the tables
// would exceed `cap_words`.
static bool conn_bitmap4(const std::vector<ConnRule4>& r, size_t cap_words, std::vector<uint32_t>& out) {
    const uint32_t R = uint32_t(r.size()), W = std::max<uint32_t>(1, (R + 31) / 32);
    auto port_in = [](uint32_t port, uint32_t pw) { return ((port - (pw & 0xFFFFu)) & 0xFFFFu) <= (pw >> 16); };
    struct Tab {
        std::vector<uint32_t> keys, rows;
    };
    // the interval starts of the six tables first (sorting 2R values each):
    // the size check needs only their counts, so a table over the cap never
    // builds its keys x R predicate rows
    auto addr_keys = [&](bool dst) {
        std::vector<uint64_t> b{0};
        for (const ConnRule4& x : r) {
            const uint32_t a = dst ? x.dst_addr : x.src_addr, m = dst ? x.dst_mask : x.src_mask;
            if (!m) continue;
            b.push_back(a);
            b.push_back(uint64_t(a) + uint64_t(~m) + 1);        // one past the prefix
        }
        std::sort(b.begin(), b.end());
        b.erase(std::unique(b.begin(), b.end()), b.end());
        while (!b.empty() && b.back() > 0xFFFFFFFFull) b.pop_back();
        return std::vector<uint32_t>(b.begin(), b.end());
    };
    auto port_keys = [&](uint32_t p) {
        std::vector<uint32_t> b{0};
        if (p < 2)
            for (const ConnRule4& x : r) {
                if (!((x.meta >> (8 * p)) & 0x80u)) continue;
                const uint32_t lo = x.port[p] & 0xFFFFu, end = lo + (x.port[p] >> 16) + 1;   // one past hi
                b.push_back(lo);
                b.push_back(end & 0xFFFFu);                      // wraps to 0 past 65535
            }
        std::sort(b.begin(), b.end());
        b.erase(std::unique(b.begin(), b.end()), b.end());
        return b;
    };
    // size (the rows are R x intervals bits); interval counts fit the
    // descriptor's 16-bit fields
    size_t words = kConnBmHeader / 4 + 2 * size_t(R);
    if (words > cap_words) return false;
    std::vector<Tab> tabs(6);
    for (int k = 0; k < 6; ++k) {
        tabs[k].keys = k < 2 ? addr_keys(k == 1) : port_keys(uint32_t(k - 2));
        words += tabs[k].keys.size() * (1 + size_t(W));
        if (words > cap_words || tabs[k].keys.size() > 0xFFFFu) return false;
    }
    // then the rows: bit i of an interval's row set when rule i's term holds
    // at the interval's first value
    for (int k = 0; k < 6; ++k) {
        Tab& t = tabs[k];
        t.rows.assign(t.keys.size() * W, 0u);
        for (size_t j = 0; j < t.keys.size(); ++j) {
            const uint32_t x = t.keys[j];
            uint32_t* row = t.rows.data() + j * W;
            for (uint32_t i = 0; i < R; ++i) {
                bool hit;
                if (k < 2) {
                    const uint32_t a = k ? r[i].dst_addr : r[i].src_addr, m = k ? r[i].dst_mask : r[i].src_mask;
                    hit = ((x ^ a) & m) == 0;
                } else {
                    const uint32_t p = uint32_t(k - 2);
                    const uint32_t pw = p == 0 ? r[i].port[0] : p == 1 ? r[i].port[1] : 0xFFFF0000u;
                    hit = ((r[i].meta >> (8 * p)) & 0x80u) && port_in(x, pw);
                }
                if (hit) row[i / 32] |= 1u << (i % 32);
            }
        }
    }
    const size_t at = out.size();
    out.insert(out.end(), {W, uint32_t(tabs[0].keys.size()), uint32_t(tabs[1].keys.size()), R,
                           uint32_t(tabs[2].keys.size()), uint32_t(tabs[3].keys.size()),
                           uint32_t(tabs[4].keys.size()), uint32_t(tabs[5].keys.size())});
    for (const Tab& t : tabs) {
        out.insert(out.end(), t.keys.begin(), t.keys.end());
        out.insert(out.end(), t.rows.begin(), t.rows.end());
    }
    for (const ConnRule4& x : r) {
        out.push_back(x.meta);
        out.push_back(x.index);
    }
    out.resize(at + ((out.size() - at + 3) & ~size_t(3)), 0u);
    return true;
}

extern "C" {

// Diagnostics (CPU tests): the connection path's bitmap form of an ACL
// (conn_bitmap4) evaluated on the host, exactly as conn_bm reads it.
int cls_conn_bitmap_eval(const cls_rule* rules, uint32_t n_rules, const uint32_t* src, const uint32_t* dst,
                         const uint16_t* dport, const uint8_t* proto, uint64_t n, uint8_t* res_out,
                         uint32_t* rule_out) {
    if ((n_rules && !rules) || (n && (!src || !dst || !dport || !proto || !res_out || !rule_out)))
        return CLS_E_INVAL;
    std::vector<SemRule> sem;
    std::string why;
    const int rc = semantic_rules(rules, n_rules, 4, sem, why);
    if (rc != CLS_OK) return rc;
    std::vector<uint32_t> w;
    if (!conn_bitmap4(conn_rules4(sem), size_t(1) << 26, w)) return CLS_E_NOMEM;
    const uint32_t W = w[0], ns = w[1], nd = w[2], np[4] = {w[4], w[5], w[6], w[7]};
    const uint32_t os = kConnBmHeader / 4, od = os + ns * (1 + W), t0 = od + nd * (1 + W);
    const uint32_t t1 = t0 + np[0] * (1 + W), t2 = t1 + np[1] * (1 + W), t3 = t2 + np[2] * (1 + W);
    const uint32_t orl = t3 + np[3] * (1 + W);
    auto row = [&](uint32_t o, uint32_t cnt, uint32_t x) {       // last key <= x (key 0 first)
        uint32_t pos = 0;
        for (uint32_t i = 1; i < cnt; ++i)
            if (w[o + i] <= x) pos = i;
        return o + cnt + W * pos;
    };
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t p = proto[k] <= 2 ? proto[k] : 3u;
        const uint32_t tp[4] = {t0, t1, t2, t3};
        const uint32_t sr = row(os, ns, src[k]), dr = row(od, nd, dst[k]), pr = row(tp[p], np[p], dport[k]);
        res_out[k] = 0;
        rule_out[k] = n_rules;
        for (uint32_t j = 0; j < W; ++j) {
            const uint32_t m = w[sr + j] & w[dr + j] & w[pr + j];
            if (m) {
                const uint32_t i = 32 * j + uint32_t(__builtin_ctz(m));
                res_out[k] = uint8_t((w[orl + 2 * i] >> (8 * p)) & 3u);
                rule_out[k] = w[orl + 2 * i + 1];
                break;
            }
        }
    }
    return CLS_OK;
}

int cls_connect_batch(cls_engine* e, const cls_conn_soa* c, uint64_t n, uint8_t* out,
                      uint32_t flags, void* stream) {
    if (!e || !c || (n && !out)) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    // host arrays: returns with the verdicts; CLS_F_DEVICE: stream-ordered
    return connect_locked(e, c, n, out, flags, stream, false);
}

int cls_connect_rules(cls_engine* e, const cls_conn_soa* c, uint64_t n, uint8_t* out, int32_t* rule_out,
                      uint32_t flags, void* stream) {
    if (!e || !c || (n && !rule_out)) return CLS_E_INVAL;
    if (flags & CLS_F_COUNT) return fail(e, CLS_E_INVAL, "cls_connect_rules does not count (CLS_F_COUNT)");
    if ((flags & CLS_F_DEVICE) && n && !aligned(rule_out, 16))
        return fail(e, CLS_E_INVAL, "device rule_out must be 16-byte aligned");
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    return connect_locked(e, c, n, out, flags, stream, false, rule_out);
}

}  // extern "C"

// The OTHER queue of a pair launch: a fixed segment per workgroup (its
// overflow is classified in place), so the buffer does not grow with the
// batch: the entries of a pair-launch workgroup (option pair_qcap: per
// wave, tests, to reach the in-place path).
static uint32_t pair_qcap(const cls_engine* e, uint64_t n, int grid) {
    if (e->opts.pair_qcap_set) return e->opts.pair_qcap * (kPairBlock / 64);
    return uint32_t(std::min<uint64_t>(pair_queue_words(n, grid), 16384));
}

// The slot -> rule map `m` of an uploaded pair image as u32 (false: no image
// then), and as u16 for the launch to stage in LDS beside the image (rules <
// 65535; padded to 8, n16 16-B units; 0: none).
static bool pair_slot_maps(const std::vector<uint32_t>& m, uint32_t n_rules, DevBuf& d_map, DevBuf& d_map16,
                           uint32_t& n16) {
    n16 = 0;
    if (d_map.ensure(std::max<size_t>(1, m.size()) * 4) != hipSuccess ||
        (!m.empty() && hipMemcpy(d_map.p, m.data(), m.size() * 4, hipMemcpyHostToDevice) != hipSuccess))
        return false;
    if (n_rules < 0xFFFFu && !m.empty()) {
        std::vector<uint16_t> m16((m.size() + 7) & ~size_t(7), 0);
        for (size_t i = 0; i < m.size(); ++i) m16[i] = uint16_t(m[i]);
        if (d_map16.ensure(m16.size() * 2) == hipSuccess &&
            hipMemcpy(d_map16.p, m16.data(), m16.size() * 2, hipMemcpyHostToDevice) == hipSuccess)
            n16 = uint32_t(m16.size() / 8);
    }
    return true;
}

// The pair launch's image of a table (Table::pimg), built and uploaded at
// its first use; false when the table has none.
static bool pair_image(cls_engine* e, Table& t) {
    if (t.pimg_state == 0) {
        t.pimg_state = -1;
        std::string why;
        const CompileScope scope(e->opts);
        if (t.sem4 && build_pair4(*t.sem4, t.n_rules, t.img.swap != 0, t.pimg, why) && t.pimg.gcells.empty() &&
            t.pimg.img_bytes + 32u <= uint32_t(max_lds_bytes()) &&
            cls_kernel_exists(t.pimg.mode, t.pimg.list_mode, true, false) &&
            upload(e, t.d_pimg, t.pimg) == CLS_OK &&
            pair_slot_maps(t.pimg.ctr_rule, t.n_rules, t.d_pslot_rule, t.d_pslot16, t.pslot16_n16))
            t.pimg_state = 1;
        if (t.pimg_state < 0) {
            t.pimg = Cls4Image();
            (void)hipGetLastError();
        }
    }
    return t.pimg_state > 0;
}

// The same for the 16-byte layout (Table::p16.pimg, compile.hpp build_pair16):
// none when the four-cell image does not fit LDS beside 32 spare bytes, has
// wide cells in global memory, or has no classify16_pair variant.
static bool pair_image16(cls_engine* e, Table& t) {
    auto& q = t.p16;
    if (q.pimg_state == 0) {
        q.pimg_state = -1;
        std::string why;
        const CompileScope scope(e->opts);
        const Cls4Image& c = q.pimg.core;
        if (q.ok && q.sem16 && build_pair16(*q.sem16, t.n_rules, q.img.core.swap != 0, q.pimg, why) &&
            c.gcells.empty() && c.img_bytes + 32u <= uint32_t(max_lds_bytes()) &&
            pair16_kernel_exists(c.mode, c.list_mode, q.pimg.src_mode) && upload(e, q.d_pimg, c) == CLS_OK &&
            pair_slot_maps(c.ctr_rule, t.n_rules, q.d_pslot_rule, q.d_pslot16, q.pslot16_n16))
            q.pimg_state = 1;
        if (q.pimg_state < 0) {
            q.pimg = Cls16Image();
            (void)hipGetLastError();
        }
    }
    return q.pimg_state > 0;
}

// ---------------------------------------------------------------------------
// A batch's resolved inputs: the arrays as the kernels see them (a device
// batch's own, a host batch's staged copies), the outputs as device pointers.
struct ConnBatch {
    const cls_conn_soa* host = nullptr;    // the caller's arrays (a host batch's plan samples them)
    bool k16 = false, dev = false, count = false;
    // the trace (cls_connect_rules): the calls' rules, no counters; it needs
    // the large ACLs' rule-bearing words as a counting batch does
    bool trace = false;
    uint64_t n = 0;
    hipStream_t s = nullptr;
    const uint32_t *sif = nullptr, *dif = nullptr;
    const void *src = nullptr, *dst = nullptr;
    const uint16_t *sp = nullptr, *dp = nullptr;
    const uint8_t* pr = nullptr;
    uint8_t* out = nullptr;
    int32_t* rule_out = nullptr;
    bool rules_wanted() const { return count || trace; }
};

// A connection scratch buffer grows only once the last stream-ordered batch
// has finished with it.
static hipError_t grow(cls_engine* e, DevBuf& d, size_t bytes) {
    if (bytes > d.bytes && conn_quiesce(e) != CLS_OK) return hipErrorUnknown;
    return d.ensure(bytes);
}

// Checks the call's arguments, orders the batch behind the last one, and
// stages host arrays on the device.
static int conn_inputs(cls_engine* e, const cls_conn_soa* c, uint64_t n, uint8_t* out, uint32_t flags,
                       void* stream, int32_t* rule_out, ConnBatch& B) {
    const cls_pkt_soa& pk = c->pkt;
    const bool k16 = pk.af == CLS_AF_V16;
    if (!k16 && pk.af != CLS_AF_V4) return fail(e, CLS_E_INVAL, "af must be CLS_AF_V4 or CLS_AF_V16");
    B.host = c;
    B.k16 = k16;
    B.src = k16 ? static_cast<const void*>(pk.src16) : pk.src4;
    B.dst = k16 ? static_cast<const void*>(pk.dst16) : pk.dst4;
    if (n && (!B.src || !B.dst || !pk.sport || !pk.dport || !pk.proto || !c->src_if || !c->dst_if))
        return fail(e, CLS_E_INVAL, "missing connection arrays");
    const bool dev = B.dev = flags & CLS_F_DEVICE;
    B.count = flags & CLS_F_COUNT;
    B.trace = rule_out != nullptr;
    B.n = n;
    const size_t ab = k16 ? 16 : 4;                       // address bytes
    // the kernels index connections with 32-bit offsets
    if (n > kClsChunk) return fail(e, CLS_E_INVAL, "connection batch above 2^30 connections");
    if (dev && k16 && n && (!aligned(B.src, 16) || !aligned(B.dst, 16)))
        return fail(e, CLS_E_INVAL, "device src16/dst16 must be 16-byte aligned");
    HIPC(e, hipSetDevice(e->device));
    hipStream_t s = B.s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    // Device batches are stream-ordered (the call returns once its launches
    // are queued, like cls_classify with CLS_F_DEVICE) and share the engine's
    // connection scratch: the last batch's stream, if another, is waited for
    // on the GPU (an event recorded on it now); a scratch buffer grows, and
    // the plan or its uploads change, only once that batch has finished.
    if (e->conn_last && e->conn_last != s) {
        if (!e->conn_sync_ev) HIPC(e, hipEventCreateWithFlags(&e->conn_sync_ev, hipEventDisableTiming));
        HIPC(e, hipEventRecord(e->conn_sync_ev, e->conn_last));
        HIPC(e, hipStreamWaitEvent(s, e->conn_sync_ev, 0));
    }
    const uint32_t n_ifs = uint32_t(e->if_acl.size());
    if (!dev)
        for (uint64_t i = 0; i < n; ++i)
            if (c->src_if[i] >= n_ifs || c->dst_if[i] >= n_ifs)
                return fail(e, CLS_E_INVAL, "connection %llu: unknown interface id", (unsigned long long)i);
    B.sif = c->src_if; B.dif = c->dst_if;
    B.sp = pk.sport; B.dp = pk.dport;
    B.pr = pk.proto;
    B.out = out;
    if (!dev && n) {
        HIPC(e, grow(e, e->s_src, n * ab)); HIPC(e, grow(e, e->s_dst, n * ab));
        HIPC(e, grow(e, e->s_if_a, n * 4)); HIPC(e, grow(e, e->s_if_b, n * 4));
        HIPC(e, grow(e, e->s_sport, n * 2)); HIPC(e, grow(e, e->s_dport, n * 2));
        HIPC(e, grow(e, e->s_proto, n)); HIPC(e, grow(e, e->s_verdict, n));
        HIPC(e, hipMemcpyAsync(e->s_src.p, B.src, n * ab, hipMemcpyHostToDevice, s));
        HIPC(e, hipMemcpyAsync(e->s_dst.p, B.dst, n * ab, hipMemcpyHostToDevice, s));
        HIPC(e, hipMemcpyAsync(e->s_if_a.p, B.sif, n * 4, hipMemcpyHostToDevice, s));
        HIPC(e, hipMemcpyAsync(e->s_if_b.p, B.dif, n * 4, hipMemcpyHostToDevice, s));
        HIPC(e, hipMemcpyAsync(e->s_sport.p, B.sp, n * 2, hipMemcpyHostToDevice, s));
        HIPC(e, hipMemcpyAsync(e->s_dport.p, B.dp, n * 2, hipMemcpyHostToDevice, s));
        HIPC(e, hipMemcpyAsync(e->s_proto.p, B.pr, n, hipMemcpyHostToDevice, s));
        B.src = e->s_src.p; B.dst = e->s_dst.p;
        B.sif = e->s_if_a.as<uint32_t>(); B.dif = e->s_if_b.as<uint32_t>();
        B.sp = e->s_sport.as<uint16_t>(); B.dp = e->s_dport.as<uint16_t>();
        B.pr = e->s_proto.as<uint8_t>(); B.out = e->s_verdict.as<uint8_t>();
    } else if (!B.out && n) {                             // a trace without verdicts: the kernel's byte goes to scratch
        HIPC(e, grow(e, e->s_verdict, n));
        B.out = e->s_verdict.as<uint8_t>();
    }
    B.rule_out = rule_out;
    if (B.trace && !dev && n) {
        HIPC(e, grow(e, e->s_trace, n * 16));
        B.rule_out = e->s_trace.as<int32_t>();
    }
    return CLS_OK;
}

// What a plan depends on besides the bindings (cls_engine::conn_gen).
struct PlanKind {
    bool k16, count, use_big, conn_cls, use_bm, trace;
    uint64_t key() const {
        return uint64_t(k16) | uint64_t(count) << 1 | uint64_t(use_big) << 2 | uint64_t(conn_cls) << 3 |
               uint64_t(use_bm) << 4 | uint64_t(trace) << 5;
    }
};
static PlanKind plan_kind(const cls_engine* e, const ConnBatch& B, uint32_t flags) {
    const bool cls_ok = B.n && !(flags & CLS_F_FORCE_LINEAR), conn_cls = flags & CLS_F_CONN_CLS;
    return {B.k16, B.count, cls_ok && (B.n >= kConnClsMinBatch || conn_cls), conn_cls,
            !B.k16 && cls_ok && e->opts.conn_bitmap, B.trace};
}

// The large ACLs of a plan.  Which: with a host batch, those whose linear
// work would be large -- connections touching the ACL x its rule count >=
// kConnClsWork x batch (touches estimated per interface binding from <= 64 Ki
// sampled connections, at hashed positions); with a device batch, the ACLs of
// >= kConnClsDevRules rules.  CLS_F_CONN_CLS: every imaged ACL.
static void plan_large_acls(const ConnBatch& B, const PlanKind& kind, size_t n_ifs, ConnPlan& P) {
    const uint64_t n = B.n;
    std::vector<uint64_t> touch(P.dtab.size(), 0);
    if (!B.dev && !kind.conn_cls) {
        const uint32_t *src_if = B.host->src_if, *dst_if = B.host->dst_if;
        const uint64_t m = std::min<uint64_t>(n, 65536);
        std::vector<uint64_t> per_if(P.ifs.size(), 0);
        for (uint64_t k = 0; k < m; ++k) {
            // sample k: a splitmix-scrambled position in stratum k (no stride aliasing)
            uint64_t z = (k + 1) * 0x9E3779B97F4A7C15ull;
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            const uint64_t lo = k * n / m, hi = (k + 1) * n / m;
            const uint64_t i = lo + z % (hi - lo);
            per_if[src_if[i]] += 1;
            if (dst_if[i] != src_if[i]) per_if[dst_if[i]] += 1;
        }
        for (size_t f = 0; f < n_ifs; ++f) {
            const uint64_t t = per_if[f] * n / m;
            if (P.ifs[f].in >= 0) touch[P.ifs[f].in] += t;
            if (P.ifs[f].out >= 0 && P.ifs[f].out != P.ifs[f].in) touch[P.ifs[f].out] += t;
        }
    }
    for (uint32_t j = 0; j < P.dtab.size(); ++j) {
        const Table& t = *P.dtab[j];
        const bool imaged = B.k16 ? t.p16.ok : t.has_cls;
        if (!imaged || t.n_rules < kConnClsMinRules) continue;
        const bool want = kind.conn_cls ||
                          (B.dev ? t.n_rules >= kConnClsDevRules
                                 : double(touch[j]) * t.n_rules >= double(kConnClsWork) * double(n));
        if (want) P.big.push_back(j);
    }
}

// IPv4: the bitmap form of the longer linear ACLs, longest first, while the
// pool (and the LDS counters when counting) still fit LDS -- a wave then pays
// a fixed number of reads per evaluation instead of its longest lane's scan
// (option conn_bitmap=0: scans only).
static void plan_bitmaps(bool count, ConnPlan& P) {
    const size_t lds_max0 = size_t(max_lds_bytes());
    // the LDS counters take their share only when they can be LDS counters
    // at all (otherwise they are global, cmode 2); no subtraction wraps
    const size_t ctr_b = count ? size_t(conn_lds_ctr_bytes(P.n_ctr)) : 0, reserve = std::min<size_t>(lds_max0 / 8, 8192);
    const size_t ctr_lds = ctr_b + reserve <= lds_max0 ? ctr_b : 0;
    const size_t cap = lds_max0 - reserve - ctr_lds;
    std::vector<size_t> order;
    for (size_t j = 0; j < P.desc.size(); ++j)
        if (P.desc[j].pre_blk < 0 && P.desc[j].n >= kConnBmMinRules) order.push_back(j);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return P.desc[a].n > P.desc[b].n; });
    std::vector<uint32_t> words;
    for (size_t j : order) {
        Table& t = *P.dtab[j];
        if (!t.conn_bm_built) {                         // once per table: rules are immutable
            if (!conn_bitmap4(t.conn4, kConnBmMaxWords, t.conn_bm)) t.conn_bm.clear();
            t.conn_bm_built = true;
        }
        const size_t used = P.pool.size() + words.size() * 4;
        if (t.conn_bm.empty() || used + t.conn_bm.size() * 4 > cap) continue;
        P.desc[j].bm_off = uint32_t(used);              // the pool is a multiple of 32 B, blobs of 16 B
        const std::vector<uint32_t>& h = t.conn_bm;     // header {W, ns, nd, nr, n0, n1, n2, n3}
        P.desc[j].bm_sd = h[1] | (h[2] << 16);
        P.desc[j].bm_tu = h[4] | (h[5] << 16);
        P.desc[j].bm_w = h[0];
        for (uint32_t len : {h[1], h[2], h[4], h[5]})   // ceil(log2(len)) steps take a table to one key
            while ((1u << P.bm_steps) < len) ++P.bm_steps;
        words.insert(words.end(), t.conn_bm.begin(), t.conn_bm.end());
    }
    const uint8_t* wb = reinterpret_cast<const uint8_t*>(words.data());
    P.pool.insert(P.pool.end(), wb, wb + words.size() * 4);
}

// The plan (ConnPlan) of a batch of `kind` over the current bindings.  Host
// work only.
static ConnPlan conn_plan_build(cls_engine* e, const ConnBatch& B, const PlanKind& kind) {
    ConnPlan P;
    const bool k16 = B.k16;
    // Snapshot the bindings: one descriptor per bound table, (in, out) per
    // interface.  Linear ACLs' compact rules go to the call's rule pool.
    std::unordered_map<int32_t, int32_t> slot;
    auto desc_of = [&](int32_t tid) -> int32_t {
        if (tid < 0) return -1;
        auto f = slot.find(tid);
        if (f != slot.end()) return f->second;
        auto t = e->tables.find(uint32_t(tid));
        if (t == e->tables.end()) return -1;
        const Table& T = *t->second;
        ConnDesc d{};
        d.pre_blk = -1;
        d.bm_off = 0xFFFFFFFFu;
        d.n = uint32_t(k16 ? T.conn16.size() : T.conn4.size());
        d.n_rules = T.n_rules;
        d.ctr_off = P.n_ctr;
        P.n_ctr += T.n_rules + 1;
        P.desc.push_back(d);
        P.dtab.push_back(t->second);
        slot[tid] = int32_t(P.desc.size() - 1);
        return int32_t(P.desc.size() - 1);
    };
    P.ifs.resize(std::max<size_t>(1, e->if_acl.size()));
    for (size_t i = 0; i < e->if_acl.size(); ++i)
        P.ifs[i] = IfAcls{desc_of(e->if_acl[i].first), desc_of(e->if_acl[i].second), -1, -1};
    // Large ACLs: the classifier evaluates the SYN tuple (src, dst, dport)
    // and the SYN-ACK tuple (dst, src, sport) of every connection in slot
    // mode (res | slot << 2 per connection); the connection kernel then
    // reads those words instead of scanning the ACL, and maps the slot to
    // its rule only for the calls testConnection makes.  Whole-batch
    // evaluation keeps the classify launches dense (no compaction).
    if (kind.use_big) plan_large_acls(B, kind, e->if_acl.size(), P);
    // the large ACLs' result-word blocks: block b = the ACL big[b], also
    // per interface (the connection kernel loads a connection's words
    // before its descriptors)
    for (size_t b = 0; b < P.big.size(); ++b) {
        ConnDesc& d = P.desc[P.big[b]];
        const Table& t = *P.dtab[P.big[b]];
        d.pre_blk = int32_t(b);
        d.n = 0;
        d.slot_rule = k16 ? t.p16.d_slot_rule.as<uint32_t>() : t.d_slot_rule.as<uint32_t>();
        for (IfAcls& f : P.ifs) {
            if (f.in == int32_t(P.big[b])) f.in_pre = int32_t(b);
            if (f.out == int32_t(P.big[b])) f.out_pre = int32_t(b);
        }
    }
    // the rule pool of the linear ACLs
    const size_t rb = k16 ? sizeof(ConnRule16) : sizeof(ConnRule4);
    for (size_t j = 0; j < P.desc.size(); ++j) {
        if (P.desc[j].pre_blk >= 0) continue;
        P.desc[j].rule_off = uint32_t(P.pool.size() / rb);
        const uint8_t* r = k16 ? reinterpret_cast<const uint8_t*>(P.dtab[j]->conn16.data())
                               : reinterpret_cast<const uint8_t*>(P.dtab[j]->conn4.data());
        P.pool.insert(P.pool.end(), r, r + size_t(P.desc[j].n) * rb);
    }
    if (kind.use_bm) plan_bitmaps(B.count, P);
    P.id = ++e->plan_ids;
    if (B.dev) {
        P.key = kind.key();
        P.gen = e->conn_gen;
    }
    return P;
}

// ---------------------------------------------------------------------------
// The large ACLs' result words: block b (the ACL big[b]) at pre + 2 b stride,
// the SYN tuple's words first, the SYN-ACK tuple's at + stride (a multiple of
// 4, so both halves stay 16-B aligned for the pair launch's stores).  In byte
// mode (res8) block b is stride bytes at pre + b stride.
struct PreFormat {
    uint64_t stride = 0;
    // When every large ACL takes a pair launch and the batch counts, the
    // launch writes each word's counter index (descriptor counter base + the
    // slot's rule) instead of its slot: the connection kernel then counts a
    // large-ACL call without a descriptor read and a dependent slot -> rule
    // gather ...
    bool rules = false;
    // ... and a batch that does not count needs only the ACLActions: one byte
    // per connection for both tuples (the words would be 8 B)
    bool res8 = false;
    // ... and a counting one u16 words when every counter index fits 14 bits
    uint32_t bytes = 4;
    size_t block() const { return size_t(res8 ? stride : 2 * stride * bytes); }
};

// The launch a large ACL takes.
enum class BigLaunch { Pair4Cells, Pair4Queue, Slots4, Pair16, Slots16 };

// Both tuples of a large ACL in one launch (classify4_pair) when the image
// is LDS-resident and the arrays allow its 16-B loads.
// A 16-byte batch takes its pair launch (classify16_pair) on the table's
// pair image alone -- there is no OTHER-queue form of it -- so the table
// qualifies only with that image (built here, at the first batch that
// could take it); its loads need the addresses 16-B aligned and 32-bit
// byte offsets into them (option conn_pair16=0: the two slot launches).
static bool pair_ok(cls_engine* e, const ConnBatch& B, Table& t) {
    if (B.k16)
        return t.p16.ok && t.p16.lds_resident && aligned(B.src, 16) && aligned(B.dst, 16) && B.n <= (1ull << 28) &&
               e->opts.conn_pair && e->opts.conn_pair16 && pair_image16(e, t);
    return t.lds_resident && aligned(B.src, 16) && aligned(B.dst, 16) && aligned(B.dp, 8) && aligned(B.sp, 8) &&
           aligned(B.pr, 4) && e->opts.conn_pair;
}

// Counting on a pair image: the slot -> rule map in LDS after the image when
// it fits (else each word's rule is a global gather).
static PairMap pair_map(const cls_engine* e, const PreFormat& F, uint32_t img_bytes, const DevBuf& d_map16,
                        uint32_t n16) {
    PairMap sm;
    sm.srl = (img_bytes + 15u) & ~15u;
    if (F.rules && n16 && e->opts.pair_map_lds && sm.srl + 16u * n16 + 32u <= uint32_t(max_lds_bytes())) {
        sm.map = d_map16.as<uint16_t>();
        sm.n16 = n16;
    } else {
        sm.srl = 0;
    }
    return sm;
}

// IPv4, the pair image: protocols > 2 in the main loop with the others -- no
// OTHER queue, drain or second image (its slots are its own: counting takes
// the counter-index words; option pair_o4=0: the OTHER queue).
static int launch_pair4_cells(cls_engine* e, const ConnBatch& B, const PreFormat& F, Table& t, uint32_t ctr_off,
                              uint32_t* pre) {
    const Cls4Dev pd = cls4_dev(t.pimg, t.d_pimg, DevBuf(), 0, t.n_rules);
    const PairMap sm = pair_map(e, F, t.pimg.img_bytes, t.d_pslot16, t.pslot16_n16);
    LaunchCfg cfg;
    cfg.stream = B.s;
    cfg.grid = cls_grid(e, true, true, sm.srl ? sm.srl + 16u * sm.n16 : t.pimg.img_bytes, B.n);
    if (e->opts.debug_conn)
        std::fprintf(stderr, "pair: pimg %u mode %u list mode %u map %u (img %u oimg %u)\n", t.pimg.img_bytes,
                     t.pimg.mode, t.pimg.list_mode, 16u * sm.n16, t.img.img_bytes, t.oimg.img_bytes);
    const Pkts4 syn{static_cast<const uint32_t*>(B.src), static_cast<const uint32_t*>(B.dst), B.dp, B.pr, B.n};
    HIPC(e, launch_classify4_pair(pd, pd, 0, framed(t.pimg, syn), B.sp, pre, F.stride, nullptr, 0,
                                  F.rules ? t.d_pslot_rule.as<uint32_t>() : nullptr, ctr_off, F.bytes, 0, false, 0u,
                                  true, sm, cfg));
    return CLS_OK;
}

// IPv4, the main image with the OTHER queue: the OTHER image beside the main
// one when both fit (no slot counters in this mode).
static int launch_pair4_queue(cls_engine* e, const ConnBatch& B, const PreFormat& F, Table& t, uint32_t ctr_off,
                              uint32_t* pre) {
    const uint64_t n = B.n;
    uint32_t o_at = (t.img.img_bytes + 15u) & ~15u;
    // (+ 32: the queue fill word after the images)
    if (o_at + t.oimg.img_bytes + 32u > uint32_t(max_lds_bytes())) o_at = 0;
    if (e->opts.pair_other_global || e->opts.pair_other_late == 2) o_at = 0;   // tests
    // else, when the OTHER image does not fit beside the main
    // one, staged over it for the drain (option
    // pair_other_late=0: read from global memory there)
    const bool o_late = !o_at && !e->opts.pair_other_global && e->opts.pair_other_late > 0 &&
                        t.oimg.img_bytes + 32u <= uint32_t(max_lds_bytes());
    Cls4Dev od = cls4_dev(t.oimg, t.d_oimg, DevBuf(), 0, t.n_rules);
    if (o_at) {
        od.off_bounds += o_at; od.off_iclass += o_at; od.off_cells += o_at;
        od.off_lists += o_at; od.off_tmpl += o_at;
    }
    LaunchCfg cfg;
    cfg.stream = B.s;
    cfg.grid = cls_grid(e, true, true, pair_queue_lds(t.img.img_bytes, o_at, t.oimg.img_bytes, o_late), n);
    // the OTHER queue, one segment per wave: its first entries
    // in the LDS left after the images (one workgroup per CU
    // either way), the rest in global memory
    // (options pair_qcap / pair_lq: entries per
    // wave in all / in LDS, tests)
    const uint32_t nwv = kPairBlock / 64;
    const uint32_t qw = (pair_qcap(e, n, cfg.grid) + nwv - 1) / nwv;
    const uint32_t q_lds = pair_queue_lds(t.img.img_bytes, o_at, t.oimg.img_bytes, o_late);
    uint32_t lq_cap = std::min<uint32_t>(qw, (uint32_t(max_lds_bytes()) - q_lds) / 16u / nwv);
    if (e->opts.pair_lq >= 0) lq_cap = std::min<uint32_t>(lq_cap, uint32_t(e->opts.pair_lq));
    const uint32_t gq = qw - lq_cap;
    HIPC(e, grow(e, e->s_pq, size_t(cfg.grid) * nwv * std::max<uint32_t>(1, gq) * 16));
    if (e->opts.debug_conn)      // diagnostics: where the OTHER image and queue live
        std::fprintf(stderr, "pair: img %u oimg %u o_at %u o_late %d lq %u gq %u cdiv %u\n",
                     t.img.img_bytes, t.oimg.img_bytes, o_at, int(o_late), lq_cap, gq,
                     e->opts.pair_class ? t.pair_cdiv : 0u);
    const Pkts4 syn{static_cast<const uint32_t*>(B.src), static_cast<const uint32_t*>(B.dst), B.dp, B.pr, n};
    HIPC(e, launch_classify4_pair(table_dev(t), od, o_at, framed(t.img, syn), B.sp, pre, F.stride,
                                  e->s_pq.as<uint32_t>(), gq, F.rules ? t.d_slot_rule.as<uint32_t>() : nullptr,
                                  ctr_off, F.bytes, lq_cap, o_late, e->opts.pair_class ? t.pair_cdiv : 0u, false,
                                  PairMap{}, cfg));
    return CLS_OK;
}

// IPv4, one slot launch per tuple.
static int launch_slots4(cls_engine* e, const ConnBatch& B, const PreFormat& F, Table& t, uint32_t* pre) {
    const Cls4Dev cd = table_dev(t);
    const uint32_t *s4 = static_cast<const uint32_t*>(B.src), *d4 = static_cast<const uint32_t*>(B.dst);
    LaunchCfg cfg;
    cfg.stream = B.s;
    cfg.other = cls4_dev(t.oimg, t.d_oimg, DevBuf(), 0, t.n_rules);
    cfg.grid = cls_grid(e, true, t.lds_resident, t.img.lds_bytes, B.n);
    HIPC(e, launch_classify4_slots(cd, framed(t.img, Pkts4{s4, d4, B.dp, B.pr, B.n}), pre, t.lds_resident, cfg));
    HIPC(e, launch_classify4_slots(cd, framed(t.img, Pkts4{d4, s4, B.sp, B.pr, B.n}), pre + F.stride,
                                   t.lds_resident, cfg));
    return CLS_OK;
}

// 16-byte layout: both tuples on the pair image in one launch
// (k16_pair.hip), written as the IPv4 pair launch writes them.
static int launch_pair16(cls_engine* e, const ConnBatch& B, const PreFormat& F, Table& t, uint32_t ctr_off,
                         uint32_t* pre) {
    auto& q = t.p16;
    const Cls4Image& pi = q.pimg.core;
    const Cls4Dev pd = cls4_dev(pi, q.d_pimg, DevBuf(), 0, t.n_rules);
    const PairMap sm = pair_map(e, F, pi.img_bytes, q.d_pslot16, q.pslot16_n16);
    LaunchCfg cfg;
    cfg.stream = B.s;
    cfg.grid = cls_grid(e, true, true, sm.srl ? sm.srl + 16u * sm.n16 : pi.img_bytes, B.n);
    if (e->opts.debug_conn)
        std::fprintf(stderr, "pair16: pimg %u mode %u list mode %u fe %u map %u (img %u oimg %u) grid %d step %u\n",
                     pi.img_bytes, pi.mode, pi.list_mode, q.pimg.src_mode, 16u * sm.n16,
                     q.img.core.img_bytes, q.oimg.img_bytes, cfg.grid, 64u * kPair16Conns);
    Pkts16 pk{static_cast<const uint4*>(B.src), static_cast<const uint4*>(B.dst), B.dp, B.pr, B.n, 0u};
    if (pi.swap) std::swap(pk.src, pk.dst);       // destination-keyed image
    HIPC(e, launch_classify16_pair(pd, fe16(q.pimg, DevBuf()), pk, B.sp, pre, F.stride,
                                   F.rules ? q.d_pslot_rule.as<uint32_t>() : nullptr, ctr_off, F.bytes, sm, cfg));
    return CLS_OK;
}

// 16-byte layout, one slot launch per tuple.
static int launch_slots16(cls_engine* e, const ConnBatch& B, const PreFormat& F, Table& t, uint32_t* pre) {
    auto& q = t.p16;
    const Cls4Image& ci = q.img.core;
    const Cls4Dev cd = cls4_dev(ci, q.d_img, q.d_lin, uint32_t(q.lin.size()), t.n_rules);
    LaunchCfg cfg;
    cfg.stream = B.s;
    cfg.other = cls4_dev(q.oimg, q.d_oimg, DevBuf(), 0, t.n_rules);
    cfg.grid = cls_grid(e, true, q.lds_resident, ci.lds_bytes, B.n);
    const Fe16 fe = fe16(q.img, q.d_src_search);
    const uint4 *s16 = static_cast<const uint4*>(B.src), *d16 = static_cast<const uint4*>(B.dst);
    Pkts16 syn{s16, d16, B.dp, B.pr, B.n, 0u}, ack{d16, s16, B.sp, B.pr, B.n, 0u};
    if (ci.swap) {                               // destination-keyed image
        std::swap(syn.src, syn.dst);
        std::swap(ack.src, ack.dst);
    }
    if (e->opts.debug_conn)
        std::fprintf(stderr, "slots16: img %u mode %u list mode %u fe %u lds %d pimg state %d\n", ci.img_bytes,
                     ci.mode, ci.list_mode, q.img.src_mode, int(q.lds_resident), q.pimg_state);
    HIPC(e, launch_classify16_slots(cd, fe, syn, pre, q.lds_resident, cfg));
    HIPC(e, launch_classify16_slots(cd, fe, ack, pre + F.stride, q.lds_resident, cfg));
    return CLS_OK;
}

// The large-ACL pass: the batch's result-word format, then each large ACL's
// launch into its block of e->s_pre.
static int conn_large_acls(cls_engine* e, const ConnBatch& B, ConnPlan& P, PreFormat& F) {
    const bool rw = B.rules_wanted();
    F.stride = (B.n + 3) & ~uint64_t(3);
    // each table's pair_ok, once per batch (P.launch: no allocation under a kept plan)
    P.launch.resize(P.big.size());
    bool all_pair = !P.big.empty();
    for (size_t b = 0; b < P.big.size(); ++b) {
        P.launch[b] = pair_ok(e, B, *P.dtab[P.big[b]]);
        all_pair = all_pair && P.launch[b];
    }
    F.rules = rw && all_pair && e->opts.conn_pre_rules;
    F.res8 = !rw && all_pair && e->opts.conn_pre_narrow;
    F.bytes = F.res8 ? 1u : F.rules && P.n_ctr <= (1u << 14) && e->opts.conn_pre_narrow ? 2u : 4u;
    if (P.big.empty()) return CLS_OK;
    HIPC(e, grow(e, e->s_pre, P.big.size() * F.block()));
    for (size_t b = 0; b < P.big.size(); ++b) {
        Table& t = *P.dtab[P.big[b]];
        const bool ok = P.launch[b], pair_words = !rw || F.rules;
        const BigLaunch kind = B.k16 ? (ok && pair_words ? BigLaunch::Pair16 : BigLaunch::Slots16)
                               : ok && e->opts.pair_o4 && pair_words && pair_image(e, t) ? BigLaunch::Pair4Cells
                               : ok ? BigLaunch::Pair4Queue : BigLaunch::Slots4;
        uint32_t* pre = reinterpret_cast<uint32_t*>(e->s_pre.as<uint8_t>() + b * F.block());
        const uint32_t ctr_off = P.desc[P.big[b]].ctr_off;
        int rc = CLS_OK;
        switch (kind) {
        case BigLaunch::Pair4Cells: rc = launch_pair4_cells(e, B, F, t, ctr_off, pre); break;
        case BigLaunch::Pair4Queue: rc = launch_pair4_queue(e, B, F, t, ctr_off, pre); break;
        case BigLaunch::Slots4: rc = launch_slots4(e, B, F, t, pre); break;
        case BigLaunch::Pair16: rc = launch_pair16(e, B, F, t, ctr_off, pre); break;
        case BigLaunch::Slots16: rc = launch_slots16(e, B, F, t, pre); break;
        }
        if (rc != CLS_OK) return rc;
    }
    return CLS_OK;
}

// ---------------------------------------------------------------------------
// The connection launch's LDS and occupancy plan, from sizes and options
// alone.  LDS: the rule pool first (every evaluation step reads it), then the
// u32 counters if they fit beside it; otherwise global-memory variants
// (option conn_no_lds, tests: bit 0 rules from global memory, bit 1 global
// counters, bit 2 descriptor / interface tables from global memory).
struct ConnLdsIn {
    size_t pool, meta, lds_max;        // rule pool, descriptor + interface tables, max_lds_bytes()
    uint32_t n_ctr;
    bool k16, count;
    uint64_t n;
    int n_cu;
    int no_lds, wg_per_cu, plan;       // options conn_no_lds, conn_wg_per_cu, conn_plan
    bool jobs, wg768;                  // options conn_jobs, conn_wg768
};
struct ConnLds {
    bool lds_rules;
    uint32_t sm_lds, ctr_lds;          // the state machine's table, the counters (ConnArgs)
    int cmode;                         // 0 no counters, 1 LDS counters, 2 global counters
    uint32_t ctr16, meta_lds, job_lds;
    int per_cu, block;
    size_t lds;
    uint64_t grid;
};
// One candidate: counters of ctr_b bytes, a shape (cap workgroups per CU, of
// `block` threads; 0: 512 when two fit, else 1024).  The descriptor and
// interface tables go after the pool and counters unless they would cost a
// workgroup per CU, then (IPv4, `jobs`) the waves' job lists (512 B per
// wave) on the same terms -- else the kernel's owner search and shuffles
// (option conn_jobs=0: tests).
static ConnLds lds_shape(const ConnLdsIn& in, const ConnLds& base, size_t ctr_b, bool jobs, int cap, int block) {
    auto per_cu_of = [&](size_t b) { return b ? std::max(1, std::min(cap, int(in.lds_max / b))) : cap; };
    ConnLds q = base;
    q.lds = base.ctr_lds + ctr_b;
    q.meta_lds = q.job_lds = 0xFFFFFFFFu;
    const size_t meta_at = (q.lds + 15) & ~size_t(15);
    if (meta_at + in.meta <= in.lds_max && per_cu_of(meta_at + in.meta) == per_cu_of(q.lds) && !(in.no_lds & 4)) {
        q.meta_lds = uint32_t(meta_at);
        q.lds = meta_at + in.meta;
    }
    q.per_cu = per_cu_of(q.lds);
    q.block = block ? block : q.per_cu >= 2 ? 512 : 1024;
    const size_t job_at = (q.lds + 15) & ~size_t(15), job_b = size_t(q.block / 64) * 512;
    if (jobs && job_at + job_b <= in.lds_max && (q.per_cu == 1 || per_cu_of(job_at + job_b) == q.per_cu)) {
        q.job_lds = uint32_t(job_at);
        q.lds = job_at + job_b;
    }
    return q;
}
// Counting with LDS counters and 16-byte addresses, the kernel holds up to
// 96 VGPRs (kernels.hip connect_kernel): at most two workgroups per CU.
// Where three 512-thread workgroups do not fit but two 768-thread ones do
// (the shared part -- pool, counters, tables -- is paid per workgroup, the
// job lists per wave), the 768-thread shape keeps 24 waves per CU instead of
// 16 (option conn_wg768=0: the 512 / 1024 shapes only).
static ConnLds lds_plan_of(const ConnLdsIn& in, const ConnLds& base, size_t ctr_b, bool jobs) {
    jobs = jobs && !in.k16 && in.jobs;
    const int cu_cap = std::min(base.cmode == 1 && in.k16 ? 2 : 3, in.wg_per_cu > 0 ? in.wg_per_cu : 3);
    // (job lists first, then waves per CU)
    auto rank = [](const ConnLds& p) { return (p.job_lds != 0xFFFFFFFFu ? 64 : 0) + p.per_cu * p.block / 64; };
    const ConnLds q = lds_shape(in, base, ctr_b, jobs, cu_cap, 0);
    if (cu_cap == 3 && in.wg768) {
        const ConnLds r = lds_shape(in, base, ctr_b, jobs, 2, 768);
        if (r.per_cu == 2 && rank(r) > rank(q)) return r;
    }
    return q;
}
static ConnLds conn_lds_plan(const ConnLdsIn& in) {
    ConnLds base{};
    base.lds_rules = in.n && in.pool && in.pool + 16 + kConnStateEntries <= in.lds_max && !(in.no_lds & 1);
    // the pool at LDS 0, then the state machine's table, then the rest
    base.sm_lds = base.lds_rules ? uint32_t((in.pool + 15) & ~size_t(15)) : 0;
    base.ctr_lds = base.sm_lds + kConnStateEntries;
    if (in.count && in.n_ctr)
        base.cmode = size_t(base.ctr_lds) + conn_lds_ctr_bytes(in.n_ctr) <= in.lds_max && !(in.no_lds & 2) ? 1 : 2;
    ConnLds plan = lds_plan_of(in, base, 0, true);
    if (base.cmode == 1) {
        // LDS counters: u32, or u16 pairs (half the LDS, a bound on a
        // workgroup's connections); with job lists (at most two workgroups
        // per CU) or without (three where the LDS allows).  Option conn_plan
        // = 32j / 16j / 32s / 16s forces one (tests, measurements).
        const size_t b32 = size_t(in.n_ctr) * 4, b16 = conn_lds_ctr_bytes(in.n_ctr);
        const ConnLds c[4] = {lds_plan_of(in, base, b32, true), lds_plan_of(in, base, b16, true),
                              lds_plan_of(in, base, b32, false), lds_plan_of(in, base, b16, false)};
        int pick = -1;
        if (in.plan >= 0) {
            pick = in.plan;
            if (c[pick].lds > in.lds_max) pick = -1;
        }
        if (pick < 0) {
            // the job lists first, then waves per CU, then u16 (12 local
            // ACLs, ms per counted batch: 16j 0.1367, 32j 0.1379, 32s 0.1468, 16s
            // 0.1571; 64: 16j 0.2289, 32 (no room for job lists) 0.2367, 16s
            // 0.2449 -- profiles/r05zh_conn_counted_plans.txt)
            auto score = [&](int k) {
                return c[k].lds > in.lds_max ? -1 : (c[k].job_lds != 0xFFFFFFFFu ? 8 : 0) +
                                                   c[k].per_cu * c[k].block / 256 + (k % 2 == 1);
            };
            pick = 0;
            for (int k = 1; k < 4; ++k)
                if (score(k) > score(pick)) pick = k;
        }
        plan = c[pick];
        plan.ctr16 = pick % 2 ? 1u : 0u;
    }
    // Persistent grid: as many 512-thread workgroups per CU as the LDS
    // allows, at most three (the kernel's registers allow 24 waves per CU);
    // else two of 768 threads, two of 512 or one of 1024.  u16 counters: at
    // most kConnWgConns connections per workgroup -- a larger batch runs k
    // full rounds of the resident grid (equal workgroups, no partial round)
    const uint64_t resident = uint64_t(in.n_cu) * plan.per_cu;
    plan.grid = std::max<uint64_t>(1, std::min<uint64_t>(resident, (in.n + plan.block - 1) / plan.block));
    if (plan.ctr16) {
        const uint64_t per_wg = uint64_t(kConnWgConns / plan.block) * plan.block;
        if (in.n > plan.grid * per_wg) plan.grid = resident * ((in.n + resident * per_wg - 1) / (resident * per_wg));
    }
    return plan;
}

// ---------------------------------------------------------------------------
// One of the call's tables, uploaded only when it differs from the last
// upload (same bindings, same batch kind: nothing to copy).
static int conn_upload(cls_engine* e, hipStream_t s, DevBuf& d, std::vector<uint8_t>& last, const void* src,
                       size_t bytes, size_t min_bytes) {
    const void* was = d.p;
    HIPC(e, grow(e, d, std::max(bytes, min_bytes)));
    const uint8_t* b = static_cast<const uint8_t*>(src);
    if (d.p == was && last.size() == bytes && (bytes == 0 || std::memcmp(last.data(), b, bytes) == 0))
        return CLS_OK;
    const int qrc = conn_quiesce(e);                 // an earlier copy may still read `last`
    if (qrc != CLS_OK) return qrc;
    last.assign(b, b + bytes);
    // from the engine's copy: it outlives the call (an unsynchronised
    // batch, sync = false, may still be copying when this returns)
    if (bytes) HIPC(e, hipMemcpyAsync(d.p, last.data(), bytes, hipMemcpyHostToDevice, s));
    return CLS_OK;
}

// The plan's tables on the device, and (counting) the call counters with the
// tables' counter pointers.
static int conn_upload_tables(cls_engine* e, const ConnBatch& B, const ConnPlan& P, int cmode, ConnArgs& a) {
    hipStream_t s = B.s;
    if (e->up_plan != P.id) {                             // a kept plan's tables are on the device already
        int rc = conn_upload(e, s, e->s_desc, e->up_desc, P.desc.data(), P.desc.size() * sizeof(ConnDesc),
                             sizeof(ConnDesc));
        if (rc == CLS_OK)
            rc = conn_upload(e, s, e->s_ifs, e->up_ifs, P.ifs.data(), P.ifs.size() * sizeof(IfAcls), sizeof(IfAcls));
        if (rc == CLS_OK) rc = conn_upload(e, s, e->s_rules, e->up_rules, P.pool.data(), P.pool.size(), 16);
        if (rc != CLS_OK) return rc;
        e->up_plan = B.dev ? P.id : ~0ull;
    }
    a.desc = e->s_desc.as<ConnDesc>();
    a.ifs = e->s_ifs.as<IfAcls>();
    a.rules = e->s_rules.p;
    if (!cmode) return CLS_OK;
    // the call counters are zero between calls (the scatter launch clears
    // what it moves); cleared here only when (re)allocated
    const size_t had = e->s_cctr.bytes;
    HIPC(e, grow(e, e->s_cctr, size_t(P.n_ctr) * 8 * kConnCtrCopies));
    if (e->s_cctr.bytes != had || !e->cctr_zero) HIPC(e, hipMemsetAsync(e->s_cctr.p, 0, e->s_cctr.bytes, s));
    // zero again only once the scatter launch (which clears what it
    // moves) is queued: an early return below forces the memset next time
    e->cctr_zero = false;
    a.ctr = e->s_cctr.as<unsigned long long>();
    std::vector<unsigned long long*> tctr;
    for (size_t j = 0; j < P.dtab.size(); ++j) {
        Table& t = *P.dtab[j];
        if (!t.d_conn_ctr.p) {
            HIPC(e, t.d_conn_ctr.ensure(size_t(t.n_rules + 1) * 8));
            HIPC(e, hipMemsetAsync(t.d_conn_ctr.p, 0, size_t(t.n_rules + 1) * 8, s));
        }
        if (t.conn_ctr_ev && s != e->stream) HIPC(e, hipStreamWaitEvent(s, t.conn_ctr_ev, 0));
        tctr.push_back(t.d_conn_ctr.as<unsigned long long>());
    }
    return conn_upload(e, s, e->s_tctr, e->up_tctr, tctr.data(), tctr.size() * sizeof(void*), sizeof(void*));
}

// The connection launch, then the flush of its counters into the tables'.
static int conn_launch(cls_engine* e, const ConnBatch& B, const ConnPlan& P, const ConnLds& L, ConnArgs& a) {
    hipStream_t s = B.s;
    const uint64_t n = B.n;
    // LDS counters leave the launch as one row per workgroup, summed into the
    // tables' counters by the rows launch (option conn_flush_atomic: device
    // atomics into the copies of the call counters and the scatter launch,
    // tests)
    const uint32_t nw = a.ctr16 ? (P.n_ctr + 1u) / 2u : P.n_ctr;
    a.ctr_rows = nullptr;
    if (L.cmode == 1 && n && !e->opts.conn_flush_atomic) {
        HIPC(e, grow(e, e->s_crows, size_t(L.grid) * nw * 4));
        a.ctr_rows = e->s_crows.as<uint32_t>();
    }
    HIPC(e, launch_connect(a, B.k16, L.lds_rules, B.trace ? 3 : L.cmode, int(L.grid), L.block, L.lds, s));
    if (L.cmode && n) {
        uint32_t max_rules = 0;
        for (const ConnDesc& d : P.desc) max_rules = std::max(max_rules, d.n_rules);
        if (a.ctr_rows) {
            HIPC(e, launch_conn_rows(a.ctr_rows, uint32_t(L.grid), nw, a.ctr16 != 0, P.n_ctr, a.desc,
                                     uint32_t(P.desc.size()), e->s_tctr.as<unsigned long long* const>(), s));
        } else {
            HIPC(e, launch_conn_scatter(a.desc, e->s_tctr.as<unsigned long long* const>(), uint32_t(P.desc.size()),
                                        max_rules, e->s_cctr.as<unsigned long long>(), kConnCtrCopies, true, P.n_ctr,
                                        s));
        }
        e->cctr_zero = true;
        // cls_conn_counters waits for this batch's scatter, not the device:
        // it reads on the engine's stream, so a batch on that stream needs no
        // event (and every earlier batch is ordered before it, conn_last);
        // one on another stream records one (an event per batch cost the
        // stream ~5 us, profiles/r06u_conn_default_12_batches.txt)
        std::shared_ptr<SharedEvent> ev;
        if (s != e->stream) {
            for (auto& x : e->conn_evs)
                if (x.use_count() == 1) {
                    ev = x;
                    break;
                }
            if (!ev) {
                ev = std::make_shared<SharedEvent>();
                HIPC(e, hipEventCreateWithFlags(&ev->ev, hipEventDisableTiming));
                e->conn_evs.push_back(ev);
            }
            HIPC(e, hipEventRecord(ev->ev, s));
        }
        for (size_t j = 0; j < P.dtab.size(); ++j) P.dtab[j]->conn_ev = ev;
    } else if (L.cmode) {
        e->cctr_zero = true;            // n == 0: nothing was counted
    }
    return CLS_OK;
}

int connect_locked(cls_engine* e, const cls_conn_soa* c, uint64_t n, uint8_t* out, uint32_t flags, void* stream,
                   bool sync, int32_t* rule_out) {
    ConnBatch B;
    int rc = conn_inputs(e, c, n, out, flags, stream, rule_out, B);
    if (rc != CLS_OK) return rc;
    // The plan (ConnPlan): a device batch reuses the last one while the
    // bindings and the flags are the same; a host batch picks its large ACLs
    // from a sample of its connections, so it plans every time.
    const PlanKind kind = plan_kind(e, B, flags);
    ConnPlan fresh;
    ConnPlan& P = B.dev ? e->conn_plan : fresh;
    if (!(B.dev && P.gen == e->conn_gen && P.key == kind.key())) {
        if (B.dev && (rc = conn_quiesce(e)) != CLS_OK) return rc;   // the kept plan's tables may be in use
        P = ConnPlan();
        P = conn_plan_build(e, B, kind);
    }
    PreFormat F;
    if ((rc = conn_large_acls(e, B, P, F)) != CLS_OK) return rc;
    const Opts& o = e->opts;
    const ConnLds L = conn_lds_plan({P.pool.size(), P.desc.size() * sizeof(ConnDesc) + P.ifs.size() * sizeof(IfAcls),
                                     size_t(max_lds_bytes()), P.n_ctr, B.k16, B.count, n, e->n_cu, o.conn_no_lds,
                                     o.conn_wg_per_cu, o.conn_plan, o.conn_jobs, o.conn_wg768});
    ConnArgs a{};
    a.n_ifs = uint32_t(e->if_acl.size());
    a.rules_bytes = uint32_t(P.pool.size());
    a.n_ctr = B.count ? P.n_ctr : 0;
    a.src_if = B.sif; a.dst_if = B.dif; a.src = B.src; a.dst = B.dst;
    a.sport = B.sp; a.dport = B.dp; a.proto = B.pr; a.n = n; a.out = B.out;
    a.rule_out = B.rule_out;
    a.sm_lds = L.sm_lds; a.ctr_lds = L.ctr_lds; a.ctr16 = L.ctr16;
    a.meta_lds = L.meta_lds; a.job_lds = L.job_lds;
    a.n_desc = uint32_t(P.desc.size());
    a.pre = P.big.empty() ? nullptr : e->s_pre.as<uint32_t>();
    a.pre_stride = F.stride;
    a.pre_rules = F.rules ? 1u : 0u;
    a.pre_bytes = F.bytes;
    a.n_big = uint32_t(P.big.size());
    a.bm_steps = P.bm_steps;
    if ((rc = conn_upload_tables(e, B, P, L.cmode, a)) != CLS_OK) return rc;
    if (o.debug_conn) {                    // diagnostics: the launch's LDS plan
        size_t nbm = 0;
        for (const ConnDesc& d : P.desc) nbm += d.bm_off != 0xFFFFFFFFu;
        std::fprintf(stderr, "connect: n %llu desc %zu big %zu bitmaps %zu pool %zu lds_rules %d ctr %u cmode %d "
                     "meta %s jobs %s lds %zu ctr16 %u per_cu %d block %d grid %llu bm_steps %u trace %d pre_rules %d "
                     "pre_bytes %u\n", (unsigned long long)n, P.desc.size(), P.big.size(), nbm, P.pool.size(),
                     int(L.lds_rules), P.n_ctr, L.cmode, L.meta_lds != 0xFFFFFFFFu ? "lds" : "global",
                     L.job_lds != 0xFFFFFFFFu ? "lds" : "shuffle", L.lds, L.ctr16, L.per_cu, L.block,
                     (unsigned long long)L.grid, P.bm_steps, int(B.trace), int(F.rules),
                     P.big.empty() ? 0u : F.bytes);
    }
    if ((rc = conn_launch(e, B, P, L, a)) != CLS_OK) return rc;
    hipStream_t s = B.s;
    if (!B.dev && n && out) HIPC(e, hipMemcpyAsync(out, B.out, n, hipMemcpyDeviceToHost, s));
    if (!B.dev && n && B.trace) HIPC(e, hipMemcpyAsync(rule_out, B.rule_out, n * 16, hipMemcpyDeviceToHost, s));
    // a host batch returns with its verdicts; a device batch is
    // stream-ordered (conn_last: its scratch is reused only behind it)
    if (sync || !B.dev) {
        HIPC(e, hipStreamSynchronize(s));
        e->conn_last = nullptr;
    } else if (n) {
        e->conn_last = s;
    }
    return CLS_OK;
}

extern "C" {

int cls_stream_floor_conn(cls_engine* e, const cls_conn_soa* c, uint64_t n, uint8_t* out, uint32_t reps,
                          float* ms, void* stream) {
    if (!e || !c || !out || !ms || c->pkt.af != CLS_AF_V4 || n < 4 || n > kClsChunk) return CLS_E_INVAL;
    const cls_pkt_soa& pk = c->pkt;
    if (!aligned(pk.src4, 16) || !aligned(pk.dst4, 16) || !aligned(c->src_if, 16) || !aligned(c->dst_if, 16) ||
        !aligned(pk.sport, 8) || !aligned(pk.dport, 8) || !aligned(pk.proto, 4) || !aligned(out, 4))
        return fail(e, CLS_E_INVAL, "cls_stream_floor_conn: device arrays must be 16/8/4-byte aligned");
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    HIPC(e, hipSetDevice(e->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    ConnArgs a{};
    a.src = pk.src4; a.dst = pk.dst4; a.src_if = c->src_if; a.dst_if = c->dst_if;
    a.sport = pk.sport; a.dport = pk.dport; a.proto = pk.proto; a.out = out; a.n = n;
    const int grid = int(std::min<uint64_t>(uint64_t(e->n_cu) * 2, (n / 4 + 1023) / 1024));
    hipEvent_t t0, t1;
    HIPC(e, hipEventCreate(&t0));
    HIPC(e, hipEventCreate(&t1));
    HIPC(e, launch_stream_conn(a, grid, s));          // warm
    HIPC(e, hipEventRecord(t0, s));
    for (uint32_t r = 0; r < std::max(1u, reps); ++r) HIPC(e, launch_stream_conn(a, grid, s));
    HIPC(e, hipEventRecord(t1, s));
    HIPC(e, hipEventSynchronize(t1));
    float t = 0.f;
    HIPC(e, hipEventElapsedTime(&t, t0, t1));
    *ms = t / float(std::max(1u, reps));
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    return CLS_OK;
}

// One device's connection counters of a table, added to `acc`: waits for
// the last counting batch's scatter and a rebind's clearing (events), not
// for other work on the device.
static int conn_counters_dev(cls_engine* d, uint32_t table_id, std::vector<uint64_t>& acc, uint32_t reset) {
    auto it = d->tables.find(table_id);
    if (it == d->tables.end()) return fail(d, CLS_E_NOTFOUND, "no table %u", table_id);
    Table& t = *it->second;
    if (!t.d_conn_ctr.p) return CLS_OK;
    HIPC(d, hipSetDevice(d->device));
    const size_t bytes = size_t(t.n_rules + 1) * 8;
    std::vector<uint64_t> h(t.n_rules + 1);
    if (t.conn_ev) HIPC(d, hipStreamWaitEvent(d->stream, t.conn_ev->ev, 0));
    if (t.conn_ctr_ev) HIPC(d, hipStreamWaitEvent(d->stream, t.conn_ctr_ev, 0));
    HIPC(d, hipMemcpyAsync(h.data(), t.d_conn_ctr.p, bytes, hipMemcpyDeviceToHost, d->stream));
    if (reset) HIPC(d, hipMemsetAsync(t.d_conn_ctr.p, 0, bytes, d->stream));
    HIPC(d, hipStreamSynchronize(d->stream));
    for (size_t i = 0; i < h.size(); ++i) acc[i] += h[i];
    return CLS_OK;
}

int cls_conn_counters(cls_engine* e, uint32_t table_id, uint64_t* counters_out, uint32_t reset) {
    if (!e || !counters_out) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    auto it = e->tables.find(table_id);
    if (it == e->tables.end()) return fail(e, CLS_E_NOTFOUND, "no table %u", table_id);
    std::vector<uint64_t> acc(size_t(it->second->n_rules) + 1, 0);
    // a multi-device engine: the sum over its devices (each counts its own
    // shard of every connection batch)
    for (size_t i = 0; i < n_dev_engines(e); ++i) {
        cls_engine* d = dev_engine(e, i);
        std::unique_lock<std::mutex> lk(d->mu, std::defer_lock);
        if (d != e) lk.lock();
        const int rc = conn_counters_dev(d, table_id, acc, reset);
        if (rc != CLS_OK) return d == e ? rc : fail(e, rc, "device %d: %s", d->device, d->err.c_str());
    }
    std::memcpy(counters_out, acc.data(), acc.size() * 8);
    return CLS_OK;
}

}  // extern "C"
