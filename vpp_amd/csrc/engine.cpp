// C ABI of the classifier engine (include/contivcls.h).
//
// Host side of the MI355X verdict backend: ACL configuration (the
// MockACLEngine's ACLConfig, mock/aclengine/aclengine_mock.go:110-121,
// 671-728), table compilation + upload, and the launch sequence of the
// classify / connection / traffic kernels on one gfx950 device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <iterator>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
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

// OTHER queue (protocols > 2 deferred to the finish launch): per workgroup
// room for 1/16 of its packets, at most 16 Ki entries (64 KiB per workgroup:
// the queue exists per (table, stream), and a full segment classifies in
// place, so a cap costs only speed on batches with > 6 % protocol > 2),
// split into one segment per wave (kOtherSegs): the entries per segment.
// Option other_cap (per workgroup): tests, to reach the in-place path.
static uint32_t other_cap(const cls_engine* e, uint64_t n, int grid) {
    if (e->opts.other_cap) return e->opts.other_cap / kOtherSegs;
    const uint64_t want = (n / uint64_t(std::max(grid, 1)) + 15) / 16;
    return uint32_t(std::min<uint64_t>(16384, std::max<uint64_t>(1024, want))) / kOtherSegs;
}

static int acl_put_locked(cls_engine* e, const char* acl_name, const cls_rule* rules, uint32_t n_rules,
                          const char* const* ingress_ifs, uint32_t n_ingress, const char* const* egress_ifs,
                          uint32_t n_egress);

extern "C" {

int cls_abi_version(void) { return CLS_ABI_VERSION; }

int cls_image_kernel(uint32_t mode, uint32_t list_mode, int lds_resident, int rep16) {
    return cls_kernel_exists(mode, list_mode, lds_resident != 0, rep16 != 0) ? CLS_OK : CLS_E_INVAL;
}

}  // extern "C"

// One device's engine (cls_engine_create, fleet.cpp, builds multi-device
// engines from these).  device < 0: the current device.
int engine_open(int dev, cls_engine** out) {
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CLS_E_NODEV;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return CLS_E_NODEV;
    if (dev >= ndev) return CLS_E_NODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return CLS_E_NODEV;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return CLS_E_NODEV;
    auto* e = new (std::nothrow) cls_engine();
    if (!e) return CLS_E_NOMEM;
    e->device = dev;
    e->n_cu = prop.multiProcessorCount;
    // The engine's stream (a call's stream == NULL) is a blocking stream: work
    // on the legacy default stream (torch's current stream unless the caller
    // set another) and the engine's calls stay ordered both ways.
    if (hipSetDevice(dev) != hipSuccess || hipStreamCreateWithFlags(&e->stream, hipStreamDefault) != hipSuccess) {
        delete e;
        return CLS_E_HIP;
    }
    *out = e;
    return CLS_OK;
}

// Waits for the engine's device work (its streams only: other engines and
// torch streams on the device are not waited for), then frees it.
void engine_close(cls_engine* e) {
    (void)hipSetDevice(e->device);
    (void)conn_quiesce(e);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->coll) (void)hipStreamSynchronize(e->coll);
    e->conn_plan = ConnPlan();
    e->tables.clear();                 // each table's Counters wait for their streams' work
    for (auto& pr : e->ev_pool) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    for (int k = 0; k < 2; ++k) {
        if (e->stage_ev[k]) (void)hipEventDestroy(e->stage_ev[k]);
        if (e->stage[k]) (void)hipHostFree(e->stage[k]);
    }
    if (e->coll) (void)hipStreamDestroy(e->coll);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

// The image, then (list modes 5, 6) its wide cells right after it: the
// kernel stages [0, img_bytes) into LDS and reads the cells from global memory.
int upload(cls_engine* e, DevBuf& d, const Cls4Image& im) {
    const size_t gb = im.gcells.size() * 4;
    HIPC(e, d.ensure(im.img_bytes + gb));
    HIPC(e, hipMemcpy(d.p, im.words.data(), im.img_bytes, hipMemcpyHostToDevice));
    if (gb) HIPC(e, hipMemcpy(static_cast<uint8_t*>(d.p) + im.img_bytes, im.gcells.data(), gb, hipMemcpyHostToDevice));
    return CLS_OK;
}

Cls4Dev cls4_dev(const Cls4Image& im, const DevBuf& d_img, const DevBuf& d_lin, uint32_t n_lin, uint32_t n_rules) {
    Cls4Dev cd;
    cd.img = d_img.as<uint32_t>();
    cd.img_bytes = im.img_bytes;
    cd.off_bounds = im.off_bounds;
    cd.off_iclass = im.off_iclass;
    cd.off_cells = im.off_cells;
    cd.off_lists = im.off_lists;
    cd.off_tmpl = im.off_tmpl;
    cd.search_top = im.search_top;
    cd.n_ctr = im.n_ctr;
    cd.lds_bytes = im.lds_bytes;
    cd.lin = d_lin.as<LinRule4>();
    cd.n_lin = n_lin;
    cd.n_rules = n_rules;
    cd.mode = im.mode;
    cd.default_row = im.default_row;
    cd.row_bytes = im.row_bytes;
    cd.port_mul = im.port_mul;
    cd.port_mask4 = im.port_mask4;
    cd.port_dflt = im.port_dflt;
    cd.n_hash = im.n_hash;
    cd.list_mode = im.list_mode;
    cd.bv_steps = std::max(im.bv_steps_d, im.bv_steps_p);  // mode 2: Sd
    cd.n_hot = im.n_hot;
    cd.off_ptop = im.off_ptop;
    cd.bv_wide = im.bv_wide;
    cd.off_hot = im.off_hot;
    cd.n_lctr = im.n_lctr;
    cd.ctr16 = im.ctr16;
    cd.off_trie = im.off_trie;
    cd.trie_depth = im.trie_depth;
    cd.gcells = im.gcells.empty() ? nullptr
                                  : reinterpret_cast<const uint8_t*>(d_img.p) + im.img_bytes;   // upload()
    cd.part = nullptr;
    cd.oq = nullptr;                 // protocols > 2 classified in place unless the caller sets a queue
    cd.oq_cap = 0;
    for (uint32_t i = 0; i < kMaxHashLens; ++i) {
        cd.hash_mask[i] = im.hash_mask[i];
        cd.hash_shift[i] = im.hash_shift[i];
        cd.hash_cap[i] = im.hash_cap[i];
        cd.hash_mul[i] = im.hash_mul[i];
        cd.hash_shift1[i] = 32u - 2u * (32u - im.hash_shift[i]);
        cd.off_hash[i] = im.off_hash[i];
    }
    return cd;
}

// Workgroups of a classify launch: persistent grid, as many per CU as LDS
// and threads allow, no more than the batch needs.
int cls_grid(const cls_engine* e, bool use_cls, bool lds_resident, uint32_t lds_bytes, uint64_t n) {
    int per_cu = 2;
    if (use_cls) {
        const int by_threads = 2048 / cls_block();
        per_cu = by_threads;
        // LDS-resident images: one 1024-thread workgroup per CU, also when two
        // would fit -- half the image stagings and counter rows, and the
        // stream runs faster in that shape (config 2: 0.0363 against 0.0392
        // ms, profiles/r04d_bench_c2{_wg1,}.json; the config-3 stream floor
        // 0.519 against 0.538 ms)
        if (lds_resident) per_cu = 1;
        if (e->opts.wg_per_cu > 0)   // diagnostics
            per_cu = std::max(1, std::min(by_threads, e->opts.wg_per_cu));
    }
    const uint64_t want = (n + 4ull * 1024 - 1) / (4ull * 1024);
    return int(std::max<uint64_t>(1, std::min<uint64_t>(uint64_t(e->n_cu) * per_cu, want)));
}

Fe16 fe16(const Cls16Image& m, const DevBuf& d_src_search) {
    Fe16 fe;
    std::memset(&fe, 0, sizeof fe);
    for (int sd = 0; sd < 2; ++sd) {
        fe.key[sd] = m.fe_key[sd];
        fe.val[sd] = m.fe_val[sd];
        fe.top[sd] = m.fe_top[sd];
        fe.k8[sd] = m.fe_k8[sd];
    }
    fe.src_mode = m.src_mode;
    if (m.src_mode == 1) {
        const uint32_t L4 = uint32_t(__builtin_ctz(m.cap4)), L6 = uint32_t(__builtin_ctz(m.cap6));
        fe.h4 = m.h4; fe.cap4 = m.cap4; fe.mul4 = m.mul4;
        fe.s4_0 = 32u - L4; fe.s4_1 = 32u - 2u * L4; fe.L4 = L4;
        fe.k6 = m.k6; fe.r6 = m.r6; fe.cap6 = m.cap6; fe.mul6 = m.mul6;
        fe.s6_0 = 32u - L6; fe.s6_1 = 32u - 2u * L6; fe.L6 = L6;
        for (int i = 0; i < 3; ++i) fe.fold[i] = m.fold[i];
        fe.dflt4 = m.dflt_row[0];
        fe.dflt6 = m.dflt_row[1];
    }
    if (m.src_mode >= 1) {                         // protocols > 2 need the rep: the global table
        fe.gsrc = d_src_search.as<uint8_t>();
        fe.gval = m.src_search_val;
        fe.gtop = m.src_search_top;
        fe.gk8 = m.src_search_k8;
    }
    return fe;
}

extern "C" {

const char* cls_last_error(const cls_engine* e) { return e ? e->err.c_str() : "null engine"; }


// ---------------------------------------------------------------------------
// The slot -> rule map of a table variant as the remap kernel reads it: every
// slot once, grouped by rule (slot order within a rule).
// Slots: the main image's, the OTHER image's, then one per rule plus the
// default DENY (the linear kernel's).
static int counters_init(cls_engine* e, Counters& c, const Cls4Image* img, const Cls4Image* oimg,
                         uint32_t n_rules) {
    const uint32_t n_cls = img ? img->n_ctr : 0, n_oth = oimg ? oimg->n_ctr : 0;
    c.n_slots = n_cls + n_oth + n_rules + 1;
    c.n_lctr = img ? img->n_lctr : 0;
    c.n_image = n_cls + n_oth;
    std::vector<uint32_t> cnt(size_t(n_rules) + 2, 0);
    auto rule_of = [&](uint32_t i) {
        return i < n_cls ? img->ctr_rule[i] : i < n_cls + n_oth ? oimg->ctr_rule[i - n_cls] : i - n_cls - n_oth;
    };
    for (uint32_t i = 0; i < c.n_slots; ++i) cnt[rule_of(i) + 1]++;
    for (size_t r = 1; r < cnt.size(); ++r) cnt[r] += cnt[r - 1];
    std::vector<uint32_t> csr(size_t(c.n_slots) * 2);
    for (uint32_t i = 0; i < c.n_slots; ++i) {
        const uint32_t r = rule_of(i), k = cnt[r]++;
        csr[2 * size_t(k)] = i;
        csr[2 * size_t(k) + 1] = r;
    }
    HIPC(e, c.d_csr.ensure(csr.size() * 4));
    HIPC(e, hipMemcpy(c.d_csr.p, csr.data(), csr.size() * 4, hipMemcpyHostToDevice));
    // slot -> rule for the finish launch.  Rules owning many slots (default
    // DENY: one no-match slot per cell; allow-all rules: one per class) are
    // "hot": a tile sums them in LDS, so such a rule takes one atomic per
    // tile instead of one per slot.
    std::vector<std::pair<uint32_t, uint32_t>> mult;            // (slots, rule)
    for (uint32_t r = 0; r <= n_rules; ++r) {
        const uint32_t m = cnt[r] - (r ? cnt[r - 1] : 0u);      // cnt[r] is now the end of rule r's run
        if (m >= 8) mult.push_back({m, r});
    }
    std::sort(mult.begin(), mult.end(), [](const auto& a, const auto& b) {
        return a.first != b.first ? a.first > b.first : a.second < b.second;
    });
    if (mult.size() > kMaxHotRules) mult.resize(kMaxHotRules);
    std::vector<uint32_t> hot_of(size_t(n_rules) + 1, 0xFFFFFFFFu);
    for (uint32_t h = 0; h < mult.size(); ++h) hot_of[mult[h].second] = h;
    std::vector<uint32_t> sr(size_t(c.n_slots) + mult.size());
    for (uint32_t i = 0; i < c.n_slots; ++i) {
        const uint32_t r = rule_of(i);
        sr[i] = hot_of[r] != 0xFFFFFFFFu ? (kHotRule | hot_of[r]) : r;
    }
    for (uint32_t h = 0; h < mult.size(); ++h) sr[c.n_slots + h] = mult[h].second;
    c.n_hot = uint32_t(mult.size());
    HIPC(e, c.d_slot_rule.ensure(sr.size() * 4));
    HIPC(e, hipMemcpy(c.d_slot_rule.p, sr.data(), sr.size() * 4, hipMemcpyHostToDevice));
    // The OTHER slots' rules, numbered compactly: the finish launch counts
    // the queued OTHER packets per rule in LDS and adds one total per
    // (workgroup, rule).  (Per slot would put many slots of one rule -- a
    // TestTraffic list's sentinel -- on one counter word from every
    // workgroup.)
    c.n_other = n_oth;
    std::vector<uint32_t> om(n_oth), orules;
    std::map<uint32_t, uint32_t> cidx;
    for (uint32_t k = 0; k < n_oth; ++k) {
        const uint32_t r = rule_of(n_cls + k);
        auto it = cidx.find(r);
        if (it == cidx.end()) {
            it = cidx.emplace(r, uint32_t(orules.size())).first;
            orules.push_back(r);
        }
        om[k] = it->second;
    }
    c.n_orules = uint32_t(orules.size());
    om.insert(om.end(), orules.begin(), orules.end());
    HIPC(e, c.d_other_map.ensure(std::max<size_t>(1, om.size()) * 4));
    if (!om.empty()) HIPC(e, hipMemcpy(c.d_other_map.p, om.data(), om.size() * 4, hipMemcpyHostToDevice));
    return CLS_OK;
}

// slot -> rule of an image and its OTHER image (slot mode of the classify
// kernels: OTHER slots follow the main image's)
static int upload_slot_rule(cls_engine* e, DevBuf& d, const Cls4Image& img, const Cls4Image& oimg) {
    std::vector<uint32_t> m(img.ctr_rule.begin(), img.ctr_rule.end());
    m.insert(m.end(), oimg.ctr_rule.begin(), oimg.ctr_rule.end());
    HIPC(e, d.ensure(std::max<size_t>(1, m.size()) * 4));
    if (!m.empty()) HIPC(e, hipMemcpy(d.p, m.data(), m.size() * 4, hipMemcpyHostToDevice));
    return CLS_OK;
}

// The rules as the caller gave them, serialised (NULL network = ""): two
// puts with equal signatures compile to the same table.
static std::string rule_sig(const cls_rule* rules, uint32_t n) {
    std::string sg;
    sg.reserve(size_t(n) * 80);
    for (uint32_t k = 0; k < n; ++k) {
        const cls_rule& r = rules[k];
        const uint32_t w[14] = {r.flags, uint32_t(r.acl_action), r.tcp_src_lo, r.tcp_src_hi, r.tcp_dst_lo,
                                r.tcp_dst_hi, r.udp_src_lo, r.udp_src_hi, r.udp_dst_lo, r.udp_dst_hi,
                                r.icmp_code_first, r.icmp_code_last, r.icmp_type_first, r.icmp_type_last};
        sg.append(reinterpret_cast<const char*>(w), sizeof w);
        sg.append(r.src_network ? r.src_network : "");
        sg.push_back('\0');
        sg.append(r.dst_network ? r.dst_network : "");
        sg.push_back('\0');
    }
    return sg;
}

// The main classifier of a rule set and its OTHER image (protocols > 2), in
// the main image's orientation.
static bool build_pair(const std::vector<SemRule>& sem, uint32_t n, Cls4Image& img, Cls4Image& oimg,
                       std::string& why) {
    if (!build_cls4(sem, n, img, why)) return false;
    return build_other4(img.swap ? swap_sides(sem) : sem, n, oimg, why);
}

// The counter scratch of (table variant, stream), created on first use.
static int scratch_of(cls_engine* e, Counters& c, uint32_t n_rules, hipStream_t s, Scratch** out);

}  // extern "C"

// A table's host form: the rules compiled once (evalACL semantics, both
// layouts, the connection path's compact rules).  No device work, so a
// multi-device engine compiles each table once and uploads it per device.
static int table_compile(cls_engine* e, const char* name, const cls_rule* rules, uint32_t n,
                         std::shared_ptr<Table>& out) {
    if (n && !rules) return fail(e, CLS_E_INVAL, "rules is NULL");
    const CompileScope scope(e->opts);      // the engine's compiler options
    auto t = std::make_shared<Table>();
    t->name = name ? name : "";
    t->n_rules = n;
    t->sig = rule_sig(rules, n);
    std::vector<SemRule> sem;
    std::string why;
    int rc = semantic_rules(rules, n, 4, sem, why);
    if (rc != CLS_OK) return fail(e, rc, "%s", why.c_str());
    t->lin4 = linear4(sem);
    t->conn4 = conn_rules4(sem);
    // rules cut off behind one that matches every packet: cls_table_need's list keeps them
    if (!sem.empty() && sem.back().index + 1 < n && matches_everything_rule(sem.back())) {
        std::vector<SemRule> all;
        rc = semantic_rules(rules, n, 4, all, why, true);
        if (rc != CLS_OK) return fail(e, rc, "%s", why.c_str());
        if (all.size() != sem.size()) t->need4 = linear4(all);
    }
    // classifier for anything but tiny tables
    t->kernel = 0;
    if (sem.size() > 8 && build_pair(sem, n, t->img, t->oimg, why)) {
        t->has_cls = true;
        t->kernel = 1;
        t->lds_resident = t->img.lds_ok && t->img.lds_bytes + kLdsReserved <= uint32_t(max_lds_bytes());
        if (t->img.h_bounds == t->oimg.h_bounds && t->img.h_iclass == t->oimg.h_iclass && t->img.row_bytes)
            t->pair_cdiv = uint32_t(((1ull << 32) + t->img.row_bytes - 1) / t->img.row_bytes);
        // the trie and wide cells exist only in LDS-resident images
        if (!cls_kernel_exists(t->img.mode, t->img.list_mode, t->lds_resident, false))
            return fail(e, CLS_E_INVAL, "no classify kernel for the compiled image (mode %u, list mode %u%s)",
                        t->img.mode, t->img.list_mode, t->lds_resident ? "" : ", global memory");
    }
    if (t->has_cls && t->lds_resident) t->sem4 = std::make_shared<const std::vector<SemRule>>(sem);
    // 16-byte layout: both families' reductions over one rep space
    auto& q = t->p16;
    std::vector<SemRule> s16;
    rc = semantic_rules(rules, n, 0, s16, why);
    if (rc != CLS_OK) return fail(e, rc, "%s", why.c_str());
    t->conn16 = conn_rules16(s16);
    for (uint32_t p = 0; p < 2; ++p) t->port_lo[p] = port_class_starts(rules, n, p);
    // each network string is parsed once: the two sides' starts, and their union (addr_class_starts(rules, n))
    for (uint32_t sd = 0; sd < 2; ++sd) t->cover_lo[sd] = cover_side_starts(rules, n, sd);
    t->addr_lo.clear();
    std::set_union(t->cover_lo[0].begin(), t->cover_lo[0].end(), t->cover_lo[1].begin(), t->cover_lo[1].end(),
                   std::back_inserter(t->addr_lo));
    std::string why16;
    q.ok = build_cls16(s16, n, q.img, why16) && build_other4(q.img.sem, n, q.oimg, why16);
    q.why = why16;
    if (q.ok) {
        const Cls4Image& c = q.img.core;
        q.lin = linear4(q.img.sem);
        q.lds_resident = c.lds_ok && c.lds_bytes + kLdsReserved <= uint32_t(max_lds_bytes());
        if (!cls_kernel_exists(c.mode, c.list_mode, q.lds_resident, true))
            return fail(e, CLS_E_INVAL, "no 16-byte classify kernel for the compiled image (mode %u, list mode %u%s)",
                        c.mode, c.list_mode, q.lds_resident ? "" : ", global memory");
        if (q.lds_resident) q.sem16 = std::make_shared<const std::vector<SemRule>>(std::move(s16));
    }
    out = std::move(t);
    return CLS_OK;
}

std::shared_ptr<Table> table_clone_host(const Table& s) {
    auto t = std::make_shared<Table>();
    t->name = s.name;
    t->n_rules = s.n_rules;
    t->sig = s.sig;
    t->lin4 = s.lin4;
    t->has_cls = s.has_cls;
    t->img = s.img;
    t->oimg = s.oimg;
    t->pair_cdiv = s.pair_cdiv;
    t->sem4 = s.sem4;                   // (the pair image is built per device, at first use)
    t->kernel = s.kernel;
    t->lds_resident = s.lds_resident;
    t->p16.ok = s.p16.ok;
    t->p16.why = s.p16.why;
    t->p16.img = s.p16.img;
    t->p16.lin = s.p16.lin;
    t->p16.oimg = s.p16.oimg;
    t->p16.lds_resident = s.p16.lds_resident;
    t->p16.sem16 = s.p16.sem16;         // (as sem4)
    t->conn4 = s.conn4;
    t->conn16 = s.conn16;
    for (int p = 0; p < 2; ++p) t->port_lo[p] = s.port_lo[p];
    t->addr_lo = s.addr_lo;
    for (int sd = 0; sd < 2; ++sd) t->cover_lo[sd] = s.cover_lo[sd];
    t->need4 = s.need4;
    t->conn_bm = s.conn_bm;
    t->conn_bm_built = s.conn_bm_built;
    t->conn_epoch = s.conn_epoch;
    return t;
}

// The device copies of a compiled table on this engine's device.
int table_upload(cls_engine* e, Table& t) {
    HIPC(e, hipSetDevice(e->device));
    HIPC(e, t.d_lin4.ensure(std::max<size_t>(1, t.lin4.size()) * sizeof(LinRule4)));
    if (!t.lin4.empty())
        HIPC(e, hipMemcpy(t.d_lin4.p, t.lin4.data(), t.lin4.size() * sizeof(LinRule4), hipMemcpyHostToDevice));
    int rc = CLS_OK;
    if (t.has_cls) {
        rc = upload(e, t.d_img, t.img);
        if (rc == CLS_OK) rc = upload(e, t.d_oimg, t.oimg);
        if (rc == CLS_OK) rc = upload_slot_rule(e, t.d_slot_rule, t.img, t.oimg);
        if (rc != CLS_OK) return rc;
    }
    rc = counters_init(e, t.c4, t.has_cls ? &t.img : nullptr, t.has_cls ? &t.oimg : nullptr, t.n_rules);
    if (rc != CLS_OK) return rc;
    auto& q = t.p16;
    if (q.ok) {
        const Cls4Image& c = q.img.core;
        rc = upload(e, q.d_img, c);
        if (rc == CLS_OK) rc = upload(e, q.d_oimg, q.oimg);
        if (rc == CLS_OK) rc = upload_slot_rule(e, q.d_slot_rule, c, q.oimg);
        if (rc != CLS_OK) return rc;
        HIPC(e, q.d_lin.ensure(std::max<size_t>(1, q.lin.size()) * sizeof(LinRule4)));
        if (!q.lin.empty())
            HIPC(e, hipMemcpy(q.d_lin.p, q.lin.data(), q.lin.size() * sizeof(LinRule4), hipMemcpyHostToDevice));
        rc = counters_init(e, t.c16, &c, &q.oimg, t.n_rules);
        if (rc != CLS_OK) return rc;
        if (q.img.src_mode >= 1) {
            HIPC(e, q.d_src_search.ensure(q.img.src_search.size() * 4));
            HIPC(e, hipMemcpy(q.d_src_search.p, q.img.src_search.data(), q.img.src_search.size() * 4,
                              hipMemcpyHostToDevice));
        }
    }
    return CLS_OK;
}

extern "C" {

// Configuration calls are made on the primary engine; a peer (a device of a
// multi-device engine, cls_device_engine) mirrors it.
static int refuse_peer(cls_engine* e) {
    return fail(e, CLS_E_INVAL, "configure a multi-device engine through its primary engine");
}

// Diagnostics and tests: one tuning switch (options.hpp) on the engine and,
// for a multi-device engine, on every device's engine.
int cls_engine_set_option(cls_engine* e, const char* key, const char* value) {
    if (!e) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    if (e->primary) return refuse_peer(e);
    std::string why;
    Opts o = e->opts;
    if (!opts_set(o, key, value, why)) return fail(e, CLS_E_INVAL, "%s", why.c_str());
    e->opts = o;
    for (cls_engine* p : e->peers) {
        std::lock_guard<std::mutex> gp(p->mu);
        p->opts = o;
    }
    // a kept connection plan was made under the old options
    e->conn_gen++;
    return sync_peers(e);
}

// A table (or a dropped binding) is gone: the kept connection plan must not
// hold its device buffers until the next device batch replans.
static void drop_conn_plan(cls_engine* e) {
    (void)conn_quiesce(e);          // a stream-ordered batch may still read the plan's tables
    e->conn_plan = ConnPlan();
    e->up_plan = ~0ull;
}

static int table_put_locked(cls_engine* e, const char* name, const cls_rule* rules, uint32_t n,
                            uint32_t* table_id) {
    std::shared_ptr<Table> t;
    int rc = table_compile(e, name, rules, n, t);
    if (rc == CLS_OK) rc = table_upload(e, *t);
    if (rc != CLS_OK) return rc;
    const uint32_t id = e->next_table++;
    e->tables[id] = t;
    e->conn_gen++;                  // connection plans see the change
    if (table_id) *table_id = id;
    return CLS_OK;
}

int cls_table_put(cls_engine* e, const char* name, const cls_rule* rules, uint32_t n_rules,
                  uint32_t* table_id) {
    if (!e) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    if (e->primary) return refuse_peer(e);
    const int rc = table_put_locked(e, name, rules, n_rules, table_id);
    return rc == CLS_OK ? sync_peers(e) : rc;
}

int cls_table_del(cls_engine* e, uint32_t table_id) {
    if (!e) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    if (e->primary) return refuse_peer(e);
    HIPC(e, hipSetDevice(e->device));
    if (!e->tables.erase(table_id)) return fail(e, CLS_E_NOTFOUND, "no table %u", table_id);
    e->conn_gen++;                  // connection plans see the change
    drop_conn_plan(e);
    return sync_peers(e);
}

int cls_table_get_info(cls_engine* e, uint32_t table_id, cls_table_info* info) {
    if (!e || !info) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    auto it = e->tables.find(table_id);
    if (it == e->tables.end()) return fail(e, CLS_E_NOTFOUND, "no table %u", table_id);
    const Table& t = *it->second;
    std::memset(info, 0, sizeof *info);
    info->n_rules = t.n_rules;
    info->kernel = uint32_t(t.kernel);
    if (t.has_cls) {
        info->lds_bytes = t.img.lds_bytes;
        info->n_intervals = t.img.n_bounds;
        info->n_classes = t.img.n_classes;
        info->n_templates = t.img.n_tmpl;
        info->n_slots = t.img.n_ctr;
        info->lds_resident = t.lds_resident ? 1 : 0;
        info->n_lctr = t.img.n_lctr;
        info->ctr16 = t.img.ctr16;
        info->list_mode = t.img.list_mode;
        info->swap = t.img.swap;
    }
    info->has_v16 = t.p16.ok ? 1u : 0u;
    if (t.p16.ok) {
        info->lds_bytes_v16 = t.p16.img.core.lds_bytes;
        info->lds_resident_v16 = t.p16.lds_resident ? 1u : 0u;
    }
    return CLS_OK;
}

// ---------------------------------------------------------------------------
// The event pair of a timed call (CLS_F_TIMING): stamped by the classify
// launch itself -- start of its first chunk's kernel, end of its last one's
// (hipExtLaunchKernel, part of the dispatch: no marker packets between the
// kernels, which cost a step several microseconds each) -- or recorded around
// the call when it has no classify launch.
static int timing_pair(cls_engine* e) {
    if (e->ev_used == e->ev_pool.size()) {
        hipEvent_t a, b;
        HIPC(e, hipEventCreate(&a));
        HIPC(e, hipEventCreate(&b));
        e->ev_pool.push_back({a, b});
    }
    e->ev0 = e->ev_pool[e->ev_used].first;
    e->ev1 = e->ev_pool[e->ev_used].second;
    e->ev_used++;
    return CLS_OK;
}

static int scratch_of(cls_engine* e, Counters& c, uint32_t n_rules, hipStream_t s, Scratch** out) {
    auto& p = c.sc[s];
    if (!p) {
        auto q = std::make_unique<Scratch>();
        HIPC(e, q->slot_val.ensure(size_t(c.n_slots) * 8));
        HIPC(e, hipMemsetAsync(q->slot_val.p, 0, size_t(c.n_slots) * 8, s));
        HIPC(e, q->out.ensure(size_t(n_rules + 1) * 8));
        // rows for the largest grid (cls_grid): never reallocated under pending work
        HIPC(e, q->part.ensure(size_t(e->n_cu) * (2048 / cls_block()) * std::max<uint32_t>(1, c.n_lctr) * 4));
        p = std::move(q);
    }
    *out = p.get();
    return CLS_OK;
}

// The OTHER queue of a launch of `grid` workgroups with segments of `cap`.
static int other_queue(cls_engine* e, Scratch* sc, int grid, uint32_t cap, hipStream_t s, uint32_t** out) {
    const size_t need = (size_t(grid) * kOtherSegs * (1 + size_t(cap))) * 4;
    if (need > sc->oq.bytes) {
        HIPC(e, hipStreamSynchronize(s));       // earlier launches on this stream may still read it
        HIPC(e, sc->oq.ensure(need));
    }
    *out = sc->oq.as<uint32_t>();
    return CLS_OK;
}

// Where a call's rule counters go, and whether they start from zero.
struct CountOut {
    unsigned long long* out;       // device rule counters (the caller's or the scratch's)
    bool zero;                     // cleared by the first fold launch
};
static CountOut count_out(Scratch* sc, uint64_t* counters_out, uint32_t flags) {
    const bool dev = flags & CLS_F_DEVICE;
    if (dev && counters_out)
        return {reinterpret_cast<unsigned long long*>(counters_out), !(flags & CLS_F_ACCUMULATE)};
    return {sc->out.as<unsigned long long>(), true};   // host batches accumulate on the host
}

// The finish launch of a classify chunk (kernels.hpp FinishArgs): fold the
// workgroups' partials, and on the last chunk move every slot to its rule.
static FinishArgs finish_args(const cls_engine* e, const Counters& c, Scratch* sc, const Cls4Dev& cd,
                              const CountOut& co, bool lds_resident, uint32_t rows, bool last) {
    FinishArgs f;
    f.part = lds_resident ? sc->part.as<uint32_t>() : nullptr;
    f.rows = rows;
    f.n_lctr = c.n_lctr;
    f.slot_val = sc->slot_val.as<unsigned long long>();
    f.n_slots = c.n_slots;
    f.slot_rule = c.d_slot_rule.as<uint32_t>();
    f.n_hot = c.n_hot;
    f.out = co.out;
    f.remap = last;
    f.oq = cd.oq;
    f.oq_rows = rows;
    f.oq_cap = cd.oq_cap;
    f.other_map = c.d_other_map.as<uint32_t>();
    f.n_other = c.n_other;
    f.n_orules = c.n_orules;
    // a tile's rows over several blocks where the tiles alone leave CUs idle
    // (option fold_split=0: one block per tile)
    const uint32_t tiles = (c.n_slots + 63u) / 64u;
    if (last && f.part && tiles && e->opts.fold_split)
        f.split = std::max(1u, std::min((rows + 63u) / 64u, uint32_t(e->n_cu) / tiles));
    return f;
}

// Slot counters -> rule counters (remap, which also clears the slots);
// host batches: copy verdicts and counters back.
static int finish_counts(cls_engine* e, const Table& t, const Counters& c, Scratch* sc, const CountOut& co,
                         uint64_t n, uint8_t* verdict_out, const uint8_t* d_verdict, uint64_t* counters_out,
                         uint32_t flags, hipStream_t s, bool remapped = false) {
    const bool dev = flags & CLS_F_DEVICE;
    if (!remapped) {
        HIPC(e, launch_remap(sc->slot_val.as<unsigned long long>(), c.d_csr.as<uint2>(), c.n_slots, co.out, s));
    }
    if (!dev) {
        if (verdict_out && n) HIPC(e, hipMemcpyAsync(verdict_out, d_verdict, n, hipMemcpyDeviceToHost, s));
        std::vector<uint64_t> tmp;
        if (counters_out) {
            tmp.resize(t.n_rules + 1);
            HIPC(e, hipMemcpyAsync(tmp.data(), co.out, tmp.size() * 8, hipMemcpyDeviceToHost, s));
        }
        HIPC(e, hipStreamSynchronize(s));
        if (counters_out) {
            for (size_t i = 0; i < tmp.size(); ++i)
                counters_out[i] = (flags & CLS_F_ACCUMULATE) ? counters_out[i] + tmp[i] : tmp[i];
        }
    }
    return CLS_OK;
}

// cls_classify of a 16-byte batch (CLS_AF_V16): front end to reps, then the
// classifier over the rep-space rules (compile.hpp Cls16Image).
static int classify16_locked(cls_engine* e, std::shared_ptr<Table> t, const cls_pkt_soa* pk, uint64_t n,
                             uint8_t* verdict_out, uint64_t* counters_out, uint32_t flags, void* stream) {
    auto& q = t->p16;
    if (!q.ok) return fail(e, CLS_E_INVAL, "no 16-byte classifier for this table: %s", q.why.c_str());
    if (n && (!pk->src16 || !pk->dst16 || !pk->dport || !pk->proto))
        return fail(e, CLS_E_INVAL, "missing packet arrays");
    if (!verdict_out && !(flags & CLS_F_NO_VERDICT) && n)
        return fail(e, CLS_E_INVAL, "verdict_out is NULL (set CLS_F_NO_VERDICT)");
    HIPC(e, hipSetDevice(e->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    const bool dev = flags & CLS_F_DEVICE;
    const uint8_t *src = pk->src16, *dst = pk->dst16, *pr = pk->proto;
    const uint16_t* dp = pk->dport;
    uint8_t* d_verdict = verdict_out;
    if (dev && n && (!aligned(src, 16) || !aligned(dst, 16)))
        return fail(e, CLS_E_INVAL, "device src16/dst16 must be 16-byte aligned");
    if (!dev && n) {
        HIPC(e, e->s_src.ensure(n * 16));
        HIPC(e, e->s_dst.ensure(n * 16));
        HIPC(e, e->s_dport.ensure(n * 2));
        HIPC(e, e->s_proto.ensure(n));
        HIPC(e, hipMemcpyAsync(e->s_src.p, src, n * 16, hipMemcpyHostToDevice, s));
        HIPC(e, hipMemcpyAsync(e->s_dst.p, dst, n * 16, hipMemcpyHostToDevice, s));
        HIPC(e, hipMemcpyAsync(e->s_dport.p, dp, n * 2, hipMemcpyHostToDevice, s));
        HIPC(e, hipMemcpyAsync(e->s_proto.p, pr, n, hipMemcpyHostToDevice, s));
        src = e->s_src.as<uint8_t>();
        dst = e->s_dst.as<uint8_t>();
        dp = e->s_dport.as<uint16_t>();
        pr = e->s_proto.as<uint8_t>();
        d_verdict = nullptr;
        if (verdict_out) {
            HIPC(e, e->s_verdict.ensure(n));
            d_verdict = e->s_verdict.as<uint8_t>();
        }
    }
    Scratch* sc = nullptr;
    {
        const int rc = scratch_of(e, t->c16, t->n_rules, s, &sc);
        if (rc != CLS_OK) return rc;
    }
    const CountOut co = count_out(sc, counters_out, flags);
    unsigned long long* slot_val = sc->slot_val.as<unsigned long long>();
    const Cls4Image& c = q.img.core;
    const bool lin = flags & CLS_F_FORCE_LINEAR;
    LaunchCfg cfg;
    cfg.stream = s;
    cfg.grid = cls_grid(e, true, q.lds_resident, c.lds_bytes, n);
    const bool timing = flags & CLS_F_TIMING;
    if (timing) {
        const int rc = timing_pair(e);
        if (rc != CLS_OK) return rc;
        if (!n) HIPC(e, hipEventRecord(e->ev0, s));
    }
    bool zeroed = false, remapped = false;
    if (n) {
        Cls4Dev cd = cls4_dev(c, q.d_img, q.d_lin, uint32_t(q.lin.size()), t->n_rules);
        cfg.other = cls4_dev(q.oimg, q.d_oimg, DevBuf(), 0, t->n_rules);
        cd.oq_cap = other_cap(e, std::min<uint64_t>(n, kClsChunk), cfg.grid);
        {
            const int rc = other_queue(e, sc, cfg.grid, cd.oq_cap, s, &cd.oq);
            if (rc != CLS_OK) return rc;
        }
        if (q.lds_resident) cd.part = sc->part.as<uint32_t>();
        Fe16 fe = fe16(q.img, q.d_src_search);
        for (uint64_t off = 0; off < n; off += kClsChunk) {
            const uint64_t m = std::min<uint64_t>(kClsChunk, n - off);
            Pkts16 pc{reinterpret_cast<const uint4*>(src + 16 * off), reinterpret_cast<const uint4*>(dst + 16 * off),
                      dp + off, pr + off, m, 0u};
            if (c.swap) std::swap(pc.src, pc.dst);          // destination-keyed image
            uint8_t* vo = d_verdict ? d_verdict + off : nullptr;
            pc.vec = aligned(pc.dport, 8) && aligned(pc.proto, 4) && (!vo || aligned(vo, 4)) ? 1u : 0u;
            cd.zero = co.zero && !zeroed ? co.out : nullptr;    // the first launch clears the call's counters
            cd.n_zero = t->n_rules + 1;
            cfg.ev_start = timing && off == 0 ? e->ev0 : nullptr;
            cfg.ev_stop = timing && off + m >= n ? e->ev1 : nullptr;
            HIPC(e, launch_classify16_cls(cd, fe, pc, vo, slot_val, q.lds_resident, lin, cfg));
            zeroed = true;
            cd.zero = nullptr;
            HIPC(e, launch_finish16(finish_args(e, t->c16, sc, cd, co, q.lds_resident, uint32_t(cfg.grid), off + m >= n),
                                    cd, cfg.other, fe, pc, vo, s));
            remapped = true;
        }
    }
    if (timing) {
        if (!n) HIPC(e, hipEventRecord(e->ev1, s));
        e->timed = true;
    }
    if (co.zero && !zeroed) HIPC(e, launch_fold(nullptr, 0, 0, slot_val, co.out, t->n_rules + 1, s));
    return finish_counts(e, *t, t->c16, sc, co, n, verdict_out, d_verdict, counters_out, flags, s, remapped);
}

}  // extern "C"

// Each packet's ACLAction and terminating rule (the debug trace of
// evalACL's matched rule, aclengine_mock.go:651-654): the classify kernels'
// slot mode, then slot -> rule; tables without a classifier image run the
// linear kernel (cls_table_cover's CLS_F_FORCE_LINEAR, `linear`: an IPv4 batch
// of any table).  No counters are touched.
int classify_rules_locked(cls_engine* e, uint32_t table_id, const cls_pkt_soa* pk, uint64_t n, uint8_t* verdict_out,
                          uint32_t* rule_out, uint32_t flags, void* stream, bool linear) {
    auto it = e->tables.find(table_id);
    if (it == e->tables.end()) return fail(e, CLS_E_NOTFOUND, "no table %u", table_id);
    const std::shared_ptr<Table> t = it->second;
    const bool v16 = pk->af == CLS_AF_V16;
    if (!v16 && pk->af != CLS_AF_V4) return fail(e, CLS_E_INVAL, "af must be CLS_AF_V4 or CLS_AF_V16");
    // table_upload leaves every 16-byte device buffer empty for such a table
    if (v16 && !t->p16.ok)
        return fail(e, CLS_E_INVAL, "no 16-byte classifier for this table: %s", t->p16.why.c_str());
    if (n && (!pk->dport || !pk->proto || (v16 ? !pk->src16 || !pk->dst16 : !pk->src4 || !pk->dst4)))
        return fail(e, CLS_E_INVAL, "missing packet arrays");
    if (n && !rule_out) return fail(e, CLS_E_INVAL, "rule_out is NULL");
    if (n > 0xFFFFFFFFull) return fail(e, CLS_E_INVAL, "batch above 2^32 packets");
    const bool dev = flags & CLS_F_DEVICE;
    const size_t ab = v16 ? 16 : 4;
    const uint8_t* src = v16 ? pk->src16 : reinterpret_cast<const uint8_t*>(pk->src4);
    const uint8_t* dst = v16 ? pk->dst16 : reinterpret_cast<const uint8_t*>(pk->dst4);
    if (dev && n && (!aligned(rule_out, 4) || (v16 && (!aligned(src, 16) || !aligned(dst, 16))) ||
                     (!v16 && (!aligned(src, 4) || !aligned(dst, 4))) || !aligned(pk->dport, 2)))
        return fail(e, CLS_E_INVAL, "device arrays must be aligned to their element size");
    HIPC(e, hipSetDevice(e->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    const uint16_t* dp = pk->dport;
    const uint8_t* pr = pk->proto;
    uint8_t* d_verdict = verdict_out;
    uint32_t* d_rule = rule_out;
    if (!dev && n) {
        HIPC(e, e->s_src.ensure(n * ab));
        HIPC(e, e->s_dst.ensure(n * ab));
        HIPC(e, e->s_dport.ensure(n * 2));
        HIPC(e, e->s_proto.ensure(n));
        HIPC(e, e->s_rule.ensure(n * 4));
        HIPC(e, hipMemcpyAsync(e->s_src.p, src, n * ab, hipMemcpyHostToDevice, s));
        HIPC(e, hipMemcpyAsync(e->s_dst.p, dst, n * ab, hipMemcpyHostToDevice, s));
        HIPC(e, hipMemcpyAsync(e->s_dport.p, dp, n * 2, hipMemcpyHostToDevice, s));
        HIPC(e, hipMemcpyAsync(e->s_proto.p, pr, n, hipMemcpyHostToDevice, s));
        src = e->s_src.as<uint8_t>();
        dst = e->s_dst.as<uint8_t>();
        dp = e->s_dport.as<uint16_t>();
        pr = e->s_proto.as<uint8_t>();
        d_rule = e->s_rule.as<uint32_t>();
        d_verdict = nullptr;
        if (verdict_out) {
            HIPC(e, e->s_verdict.ensure(n));
            d_verdict = e->s_verdict.as<uint8_t>();
        }
    }
    LaunchCfg cfg;
    cfg.stream = s;
    for (uint64_t off = 0; off < n; off += kClsChunk) {        // 32-bit packet offsets in the kernels
        const uint64_t m = std::min<uint64_t>(kClsChunk, n - off);
        uint8_t* vo = d_verdict ? d_verdict + off : nullptr;
        uint32_t* ro = d_rule + off;
        if (v16) {
            const auto& q = t->p16;
            const Cls4Image& ci = q.img.core;
            const Cls4Dev cd = cls4_dev(ci, q.d_img, q.d_lin, uint32_t(q.lin.size()), t->n_rules);
            cfg.other = cls4_dev(q.oimg, q.d_oimg, DevBuf(), 0, t->n_rules);
            cfg.grid = cls_grid(e, true, q.lds_resident, ci.lds_bytes, m);
            Pkts16 pc{reinterpret_cast<const uint4*>(src + 16 * off), reinterpret_cast<const uint4*>(dst + 16 * off),
                      dp + off, pr + off, m, 0u};
            if (ci.swap) std::swap(pc.src, pc.dst);          // destination-keyed image
            HIPC(e, launch_classify16_slots(cd, fe16(q.img, q.d_src_search), pc, ro, q.lds_resident, cfg));
            HIPC(e, launch_slot_rules(ro, q.d_slot_rule.as<uint32_t>(), uint32_t(m), vo, ro, s));
        } else {
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src) + off;
            const uint32_t* d4 = reinterpret_cast<const uint32_t*>(dst) + off;
            const Pkts4 pc{s4, d4, dp + off, pr + off, m};
            if (t->has_cls && !linear) {
                cfg.other = cls4_dev(t->oimg, t->d_oimg, DevBuf(), 0, t->n_rules);
                cfg.grid = cls_grid(e, true, t->lds_resident, t->img.lds_bytes, m);
                HIPC(e, launch_classify4_slots(table_dev(*t), framed(t->img, pc), ro, t->lds_resident, cfg));
                HIPC(e, launch_slot_rules(ro, t->d_slot_rule.as<uint32_t>(), uint32_t(m), vo, ro, s));
            } else {
                cfg.grid = cls_grid(e, false, false, 0, m);
                HIPC(e, launch_classify4_linear(t->d_lin4.as<LinRule4>(), uint32_t(t->lin4.size()), t->n_rules, pc,
                                                vo, nullptr, cfg, ro));
            }
        }
    }
    if (!dev && n) {
        if (verdict_out) HIPC(e, hipMemcpyAsync(verdict_out, d_verdict, n, hipMemcpyDeviceToHost, s));
        HIPC(e, hipMemcpyAsync(rule_out, d_rule, n * 4, hipMemcpyDeviceToHost, s));
        HIPC(e, hipStreamSynchronize(s));
    }
    return CLS_OK;
}

extern "C" {

int cls_classify_rules(cls_engine* e, uint32_t table_id, const cls_pkt_soa* pk, uint64_t n, uint8_t* verdict_out,
                       uint32_t* rule_out, uint32_t flags, void* stream) {
    if (!e || !pk) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    return classify_rules_locked(e, table_id, pk, n, verdict_out, rule_out, flags, stream);
}

int cls_classify(cls_engine* e, uint32_t table_id, const cls_pkt_soa* pk, uint64_t n,
                 uint8_t* verdict_out, uint64_t* counters_out, uint32_t flags, void* stream) {
    if (!e || !pk) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    return classify_locked(e, table_id, pk, n, verdict_out, counters_out, flags, stream);
}

}  // extern "C"

int classify_locked(cls_engine* e, uint32_t table_id, const cls_pkt_soa* pk, uint64_t n,
                    uint8_t* verdict_out, uint64_t* counters_out, uint32_t flags, void* stream) {
    auto it = e->tables.find(table_id);
    if (it == e->tables.end()) return fail(e, CLS_E_NOTFOUND, "no table %u", table_id);
    std::shared_ptr<Table> t = it->second;
    if (pk->af == CLS_AF_V16) return classify16_locked(e, t, pk, n, verdict_out, counters_out, flags, stream);
    if (pk->af != CLS_AF_V4) return fail(e, CLS_E_INVAL, "af must be CLS_AF_V4 or CLS_AF_V16");
    if (n && (!pk->src4 || !pk->dst4 || !pk->dport || !pk->proto))
        return fail(e, CLS_E_INVAL, "missing packet arrays");
    if (!verdict_out && !(flags & CLS_F_NO_VERDICT) && n)
        return fail(e, CLS_E_INVAL, "verdict_out is NULL (set CLS_F_NO_VERDICT)");
    HIPC(e, hipSetDevice(e->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    const bool dev = flags & CLS_F_DEVICE;

    Pkts4 p{pk->src4, pk->dst4, pk->dport, pk->proto, n};
    uint8_t* d_verdict = verdict_out;
    if (!dev && n) {
        HIPC(e, e->s_src.ensure(n * 4));
        HIPC(e, e->s_dst.ensure(n * 4));
        HIPC(e, e->s_dport.ensure(n * 2));
        HIPC(e, e->s_proto.ensure(n));
        HIPC(e, hipMemcpyAsync(e->s_src.p, pk->src4, n * 4, hipMemcpyHostToDevice, s));
        HIPC(e, hipMemcpyAsync(e->s_dst.p, pk->dst4, n * 4, hipMemcpyHostToDevice, s));
        HIPC(e, hipMemcpyAsync(e->s_dport.p, pk->dport, n * 2, hipMemcpyHostToDevice, s));
        HIPC(e, hipMemcpyAsync(e->s_proto.p, pk->proto, n, hipMemcpyHostToDevice, s));
        p = Pkts4{e->s_src.as<uint32_t>(), e->s_dst.as<uint32_t>(), e->s_dport.as<uint16_t>(),
                  e->s_proto.as<uint8_t>(), n};
        d_verdict = nullptr;
        if (verdict_out) {
            HIPC(e, e->s_verdict.ensure(n));
            d_verdict = e->s_verdict.as<uint8_t>();
        }
    }
    Scratch* sc = nullptr;
    {
        const int rc = scratch_of(e, t->c4, t->n_rules, s, &sc);
        if (rc != CLS_OK) return rc;
    }
    const CountOut co = count_out(sc, counters_out, flags);
    unsigned long long* slot_val = sc->slot_val.as<unsigned long long>();

    const bool vec = aligned(p.src, 16) && aligned(p.dst, 16) && aligned(p.dport, 8) &&
                     aligned(p.proto, 4) && (!d_verdict || aligned(d_verdict, 4));
    LaunchCfg cfg;
    cfg.stream = s;
    const bool use_cls = t->has_cls && !(flags & CLS_F_FORCE_LINEAR);
    cfg.grid = cls_grid(e, use_cls, t->lds_resident, t->img.lds_bytes, n);

    const bool timing = flags & CLS_F_TIMING;
    if (timing) {
        const int rc = timing_pair(e);
        if (rc != CLS_OK) return rc;
        if (!(n && use_cls)) HIPC(e, hipEventRecord(e->ev0, s));
    }
    bool zeroed = false, remapped = false;
    if (n) {
        if (use_cls) {
            Cls4Dev cd = table_dev(*t);
            cfg.other = cls4_dev(t->oimg, t->d_oimg, DevBuf(), 0, t->n_rules);
            cd.oq_cap = other_cap(e, std::min<uint64_t>(n, kClsChunk), cfg.grid);
            {
                const int rc = other_queue(e, sc, cfg.grid, cd.oq_cap, s, &cd.oq);
                if (rc != CLS_OK) return rc;
            }
            if (t->lds_resident) cd.part = sc->part.as<uint32_t>();
            // the kernel indexes packets with 32-bit offsets: chunks of 2^30
            for (uint64_t off = 0; off < n; off += kClsChunk) {
                const uint64_t m = std::min<uint64_t>(kClsChunk, n - off);
                const Pkts4 pc = framed(t->img, Pkts4{p.src + off, p.dst + off, p.dport + off, p.proto + off, m});
                uint8_t* vo = d_verdict ? d_verdict + off : nullptr;
                cd.zero = co.zero && !zeroed ? co.out : nullptr;   // the first launch clears the call's counters
                cd.n_zero = t->n_rules + 1;
                cfg.ev_start = timing && off == 0 ? e->ev0 : nullptr;
                cfg.ev_stop = timing && off + m >= n ? e->ev1 : nullptr;
                HIPC(e, launch_classify4_cls(cd, pc, vo, slot_val, t->lds_resident, vec, cfg));
                zeroed = true;
                cd.zero = nullptr;
                FinishArgs fa = finish_args(e, t->c4, sc, cd, co, t->lds_resident, uint32_t(cfg.grid), off + m >= n);
                fa.qmask = 1u;                      // the IPv4 launch's queue entries (run_n kMaskQ)
                HIPC(e, launch_finish4(fa, cfg.other, pc, vo, s));
                remapped = true;
            }
        } else {
            const uint32_t base = t->c4.n_image;
            HIPC(e, launch_classify4_linear(t->d_lin4.as<LinRule4>(), uint32_t(t->lin4.size()), t->n_rules, p,
                                            d_verdict, slot_val + base, cfg));
        }
    }
    if (timing) {
        // ev0 / ev1: the classify kernel's own start and end (stamped by its
        // launch, before the fold of the workgroup partials)
        if (!(n && use_cls)) HIPC(e, hipEventRecord(e->ev1, s));
        e->timed = true;
    }
    if (co.zero && !zeroed) HIPC(e, launch_fold(nullptr, 0, 0, slot_val, co.out, t->n_rules + 1, s));
    return finish_counts(e, *t, t->c4, sc, co, n, verdict_out, d_verdict, counters_out, flags, s, remapped);
}

extern "C" {

// Each stream shape's time (cls_stream_floor_shapes): shape = variant << 1 |
// (two workgroups per CU), 8 shapes for the IPv4 layout, 2 for the 16-byte one.
static int stream_shapes(cls_engine* e, const cls_pkt_soa* pk, uint64_t n, uint8_t* verdict, uint32_t reps,
                         std::vector<float>& out, void* stream) {
    if (!e || !pk || !verdict || n == 0 || n > kClsChunk) return CLS_E_INVAL;
    HIPC(e, hipSetDevice(e->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    Pkts4 p4{pk->src4, pk->dst4, pk->dport, pk->proto, n};
    Pkts16 p16{reinterpret_cast<const uint4*>(pk->src16), reinterpret_cast<const uint4*>(pk->dst16), pk->dport,
               pk->proto, n, 1u};
    const bool v4 = pk->af == CLS_AF_V4;
    if (v4 ? !(aligned(pk->src4, 16) && aligned(pk->dst4, 16) && aligned(pk->dport, 8) && aligned(pk->proto, 4) &&
               aligned(verdict, 4))
           : !(pk->af == CLS_AF_V16 && aligned(pk->src16, 16) && aligned(pk->dst16, 16)))
        return fail(e, CLS_E_INVAL, "stream floor: device arrays of the classify kernel's alignment");
    // the floor is the fastest of the stream shapes: one or two 1024-thread
    // workgroups per CU (the classify kernel runs one when its LDS image
    // takes more than half the CU's LDS), loads one step ahead or not, the
    // protocol stream non-temporal or cached
    hipEvent_t a, b;
    HIPC(e, hipEventCreate(&a));
    HIPC(e, hipEventCreate(&b));
    int rc = CLS_OK;
    const uint32_t k = std::max<uint32_t>(1, reps);
    const bool dbg = e->opts.debug_floor;
    out.clear();
    for (int shape = 0; shape < (v4 ? 8 : 2) && rc == CLS_OK; ++shape) {
        const int grid = e->n_cu * (1 + (shape & 1)), variant = shape >> 1;
        for (uint32_t i = 0; i <= k && rc == CLS_OK; ++i) {   // launch 0: warm-up
            if (i == 1 && hipEventRecord(a, s) != hipSuccess) rc = CLS_E_HIP;
            if (rc == CLS_OK &&
                launch_stream(v4 ? &p4 : nullptr, v4 ? nullptr : &p16, verdict, grid, variant, s) != hipSuccess)
                rc = fail(e, CLS_E_HIP, "stream floor launch failed");
        }
        float t = 0.0f;
        if (rc == CLS_OK && hipEventRecord(b, s) == hipSuccess && hipEventSynchronize(b) == hipSuccess &&
            hipEventElapsedTime(&t, a, b) == hipSuccess) {
            t /= float(k);
            if (dbg) std::fprintf(stderr, "stream floor: grid %d variant %d: %.4f ms\n", grid, variant, t);
            out.push_back(t);
        } else if (rc == CLS_OK) {
            rc = fail(e, CLS_E_HIP, "stream floor timing failed");
        }
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return rc;
}

int cls_stream_floor(cls_engine* e, const cls_pkt_soa* pk, uint64_t n, uint8_t* verdict, uint32_t reps,
                     float* ms, void* stream) {
    if (!e || !ms) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    std::vector<float> t;
    const int rc = stream_shapes(e, pk, n, verdict, reps, t, stream);
    if (rc != CLS_OK) return rc;
    *ms = *std::min_element(t.begin(), t.end());
    return CLS_OK;
}

int cls_stream_floor_shapes(cls_engine* e, const cls_pkt_soa* pk, uint64_t n, uint8_t* verdict, uint32_t reps,
                            float* ms, uint32_t cap, uint32_t* count, void* stream) {
    if (!e || !count || (cap && !ms)) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    std::vector<float> t;
    const int rc = stream_shapes(e, pk, n, verdict, reps, t, stream);
    if (rc != CLS_OK) return rc;
    *count = uint32_t(t.size());
    std::copy(t.begin(), t.begin() + std::min<size_t>(cap, t.size()), ms);
    return CLS_OK;
}

int cls_last_kernel_ms(cls_engine* e, float* ms) {
    if (!e || !ms) return CLS_E_INVAL;
    // the pair of the last timed call, read under the mutex: a concurrent timed
    // call hands out and records a new pair inside its own locked section
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    if (!e->timed) return fail(e, CLS_E_INVAL, "no timed classify recorded");
    HIPC(e, hipSetDevice(e->device));
    HIPC(e, hipEventSynchronize(e->ev1));
    HIPC(e, hipEventElapsedTime(ms, e->ev0, e->ev1));
    return CLS_OK;
}

int cls_kernel_times(cls_engine* e, float* ms, uint32_t cap, uint32_t* count) {
    if (!e || !count) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    *count = uint32_t(e->ev_used);
    if (e->ev_used == 0) return CLS_OK;
    // every pair's end: timed calls on several streams finish in any order
    for (size_t i = 0; i < e->ev_used; ++i) HIPC(e, hipEventSynchronize(e->ev_pool[i].second));
    for (size_t i = 0; i < e->ev_used && i < cap && ms; ++i)
        HIPC(e, hipEventElapsedTime(&ms[i], e->ev_pool[i].first, e->ev_pool[i].second));
    return CLS_OK;
}

int cls_kernel_starts(cls_engine* e, float* ms, uint32_t cap, uint32_t* count) {
    if (!e || !count) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    *count = uint32_t(e->ev_used);
    if (e->ev_used == 0) return CLS_OK;
    // every pair's end: timed calls on several streams finish in any order
    for (size_t i = 0; i < e->ev_used; ++i) HIPC(e, hipEventSynchronize(e->ev_pool[i].second));
    for (size_t i = 0; i < e->ev_used && i < cap && ms; ++i)
        HIPC(e, hipEventElapsedTime(&ms[i], e->ev_pool[0].first, e->ev_pool[i].first));
    return CLS_OK;
}

int cls_kernel_times_reset(cls_engine* e) {
    if (!e) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    for (size_t i = 0; i < e->ev_used; ++i) HIPC(e, hipEventSynchronize(e->ev_pool[i].second));
    e->ev_used = 0;
    return CLS_OK;
}

// ---------------------------------------------------------------------------
// ACLConfig
static uint32_t if_id_locked(cls_engine* e, const std::string& name) {
    auto it = e->if_ids.find(name);
    if (it != e->if_ids.end()) return it->second;
    const uint32_t id = uint32_t(e->if_names.size());
    e->if_ids[name] = id;
    e->if_names.push_back(name);
    e->if_acl.push_back({-1, -1});
    e->conn_gen++;                  // connection plans see the change
    return id;
}

static int acl_del_locked(cls_engine* e, const std::string& name) {
    auto it = e->acls.find(name);
    if (it == e->acls.end()) return fail(e, CLS_E_NOTFOUND, "cannot find ACL: %s", name.c_str());
    const int32_t tid = int32_t(it->second.table_id);
    (void)hipSetDevice(e->device);
    for (auto& b : e->if_acl) {
        if (b.first == tid) b.first = -1;
        if (b.second == tid) b.second = -1;
    }
    e->tables.erase(it->second.table_id);
    e->conn_gen++;                  // connection plans see the change
    drop_conn_plan(e);
    e->acls.erase(it);
    e->changes++;
    return CLS_OK;
}

int cls_acl_put(cls_engine* e, const char* acl_name, const cls_rule* rules, uint32_t n_rules,
                const char* const* ingress_ifs, uint32_t n_ingress, const char* const* egress_ifs,
                uint32_t n_egress) {
    if (!e || !acl_name) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    if (e->primary) return refuse_peer(e);
    const int rc = acl_put_locked(e, acl_name, rules, n_rules, ingress_ifs, n_ingress, egress_ifs, n_egress);
    return rc == CLS_OK ? sync_peers(e) : rc;
}

}  // extern "C"

static int acl_put_locked(cls_engine* e, const char* acl_name, const cls_rule* rules, uint32_t n_rules,
                          const char* const* ingress_ifs, uint32_t n_ingress, const char* const* egress_ifs,
                          uint32_t n_egress) {
    if (n_ingress + n_egress == 0) return fail(e, CLS_E_INVAL, "ACL with empty interfaces");
    if (n_rules && !rules) return fail(e, CLS_E_INVAL, "rules is NULL");
    const std::string name(acl_name);
    uint32_t tid;
    auto old = e->acls.find(name);
    auto same = old == e->acls.end() ? e->tables.end() : e->tables.find(old->second.table_id);
    if (same != e->tables.end() && same->second->sig == rule_sig(rules, n_rules)) {
        // Equal rules (the renderer re-puts a table whose pods changed,
        // acl_renderer.go:186-190): keep the compiled table, move the bindings.
        // A put installs a new ACL (PutACL replaces the message,
        // aclengine_mock.go:707-713), so its connection counters start from
        // zero either way.  Every connection batch has finished its work on
        // them (cls_connect_batch synchronises its stream before it returns,
        // under this mutex), so the clearing is queued on the engine stream
        // without waiting; a later counting batch on another stream waits for
        // the event recorded behind it.
        tid = old->second.table_id;
        Table& kt = *same->second;
        if (kt.d_conn_ctr.p) {
            const int qrc = conn_quiesce(e);           // a counting batch on another stream may still add
            if (qrc != CLS_OK) return qrc;
            (void)hipSetDevice(e->device);
            HIPC(e, hipMemsetAsync(kt.d_conn_ctr.p, 0, size_t(kt.n_rules + 1) * 8, e->stream));
            if (!kt.conn_ctr_ev) HIPC(e, hipEventCreateWithFlags(&kt.conn_ctr_ev, hipEventDisableTiming));
            HIPC(e, hipEventRecord(kt.conn_ctr_ev, e->stream));
        }
        kt.conn_epoch++;                // a multi-device engine's peers clear their copies
        for (auto& b : e->if_acl) {
            if (b.first == int32_t(tid)) b.first = -1;
            if (b.second == int32_t(tid)) b.second = -1;
        }
        e->acls.erase(old);
        e->rebinds++;
    } else {
        int rc = table_put_locked(e, acl_name, rules, n_rules, &tid);
        if (rc != CLS_OK) return rc;
        if (old != e->acls.end()) {         // PutACL: delete the original first, not a change
            acl_del_locked(e, name);
            e->changes--;
        }
        e->compiles++;
    }
    AclEntry a;
    a.table_id = tid;
    for (uint32_t i = 0; i < n_ingress; ++i) {
        const uint32_t id = if_id_locked(e, ingress_ifs[i]);
        a.ingress.push_back(id);
        e->if_acl[id].first = int32_t(tid);
        e->conn_gen++;                  // connection plans see the change
    }
    for (uint32_t i = 0; i < n_egress; ++i) {
        const uint32_t id = if_id_locked(e, egress_ifs[i]);
        a.egress.push_back(id);
        e->if_acl[id].second = int32_t(tid);
        e->conn_gen++;                  // connection plans see the change
    }
    e->acls[name] = a;
    e->changes++;
    return CLS_OK;
}

extern "C" {

int cls_acl_stats(cls_engine* e, uint32_t* n_compiles, uint32_t* n_rebinds) {
    if (!e) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    if (n_compiles) *n_compiles = e->compiles;
    if (n_rebinds) *n_rebinds = e->rebinds;
    return CLS_OK;
}

int cls_acl_del(cls_engine* e, const char* acl_name) {
    if (!e || !acl_name) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    if (e->primary) return refuse_peer(e);
    const int rc = acl_del_locked(e, acl_name);
    return rc == CLS_OK ? sync_peers(e) : rc;
}

int cls_acl_table(cls_engine* e, const char* acl_name, uint32_t* table_id) {
    if (!e || !acl_name || !table_id) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    auto it = e->acls.find(acl_name);
    if (it == e->acls.end()) return fail(e, CLS_E_NOTFOUND, "cannot find ACL: %s", acl_name);
    *table_id = it->second.table_id;
    return CLS_OK;
}

int cls_acl_counts(cls_engine* e, uint32_t* n_acls, uint32_t* n_changes) {
    if (!e) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    if (n_acls) *n_acls = uint32_t(e->acls.size());
    if (n_changes) *n_changes = e->changes;
    return CLS_OK;
}

int cls_if_id(cls_engine* e, const char* if_name, uint32_t* id) {
    if (!e || !if_name || !id) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    if (e->primary) return refuse_peer(e);
    *id = if_id_locked(e, if_name);
    return sync_peers(e);
}

int cls_if_acls(cls_engine* e, uint32_t if_id, int32_t* in_table, int32_t* out_table) {
    if (!e) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    if (if_id >= e->if_acl.size()) return fail(e, CLS_E_NOTFOUND, "no interface %u", if_id);
    if (in_table) *in_table = e->if_acl[if_id].first;
    if (out_table) *out_table = e->if_acl[if_id].second;
    return CLS_OK;
}

// ---------------------------------------------------------------------------
int cls_gen_traffic_v4(cls_engine* e, const cls_traffic_spec* sp, uint64_t first, uint64_t n,
                       uint32_t* src4, uint32_t* dst4, uint16_t* sport, uint16_t* dport,
                       uint8_t* proto, void* stream) {
    if (!e || !sp) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    return gen4_locked(e, sp, first, n, src4, dst4, sport, dport, proto, stream, true);
}

}  // extern "C"

int gen4_locked(cls_engine* e, const cls_traffic_spec* sp, uint64_t first, uint64_t n, uint32_t* src4,
                uint32_t* dst4, uint16_t* sport, uint16_t* dport, uint8_t* proto, void* stream, bool sync) {
    HIPC(e, hipSetDevice(e->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    const size_t bp = size_t(sp->n_pod_ips) * 4, bd = size_t(sp->n_dst) * 4, bl = sp->n_dst,
                 bq = size_t(sp->n_ports) * 2;
    auto al = [](size_t x) { return (x + 15) & ~size_t(15); };
    HIPC(e, e->s_pool.ensure(al(bp) + al(bd) + al(bl) + al(bq) + 16));
    uint8_t* base = e->s_pool.as<uint8_t>();
    TrafficDev t;
    t.seed = sp->seed;
    t.pct_pod = sp->pct_pod_src; t.pct_dst = sp->pct_rule_dst;
    t.pct_port = sp->pct_table_port; t.pct_icmp = sp->pct_icmp;
    t.pods = reinterpret_cast<const uint32_t*>(base); t.n_pods = sp->n_pod_ips;
    t.dst_addrs = reinterpret_cast<const uint32_t*>(base + al(bp));
    t.dst_lens = base + al(bp) + al(bd); t.n_dst = sp->n_dst;
    t.ports = reinterpret_cast<const uint16_t*>(base + al(bp) + al(bd) + al(bl)); t.n_ports = sp->n_ports;
    if (bp) HIPC(e, hipMemcpyAsync(base, sp->pod_ips, bp, hipMemcpyHostToDevice, s));
    if (bd) HIPC(e, hipMemcpyAsync(base + al(bp), sp->dst_addrs, bd, hipMemcpyHostToDevice, s));
    if (bl) HIPC(e, hipMemcpyAsync(base + al(bp) + al(bd), sp->dst_lens, bl, hipMemcpyHostToDevice, s));
    if (bq) HIPC(e, hipMemcpyAsync(base + al(bp) + al(bd) + al(bl), sp->ports, bq, hipMemcpyHostToDevice, s));
    HIPC(e, launch_gen4(t, first, n, src4, dst4, sport, dport, proto, s));
    // the pools are engine scratch (sync = false: the caller synchronises
    // before the next use)
    if (sync) HIPC(e, hipStreamSynchronize(s));
    return CLS_OK;
}

extern "C" {

// Blob of cls_compile_v4 / cls_compile_v16: header (v4 header, then `extra`
// bytes of a larger header), image, slot -> rule map, linear rules.
static int write_blob(const Cls4Image* img, const std::vector<LinRule4>& lin, uint32_t n, uint32_t magic,
                      const void* extra, size_t extra_bytes, void* blob, uint64_t cap, uint64_t* need,
                      const std::vector<uint32_t>* trailer = nullptr, size_t trailer_field = 0,
                      const Cls4Image* other = nullptr) {
    cls_image_v4_header h;
    std::memset(&h, 0, sizeof h);
    h.magic = magic;
    h.version = 4;
    h.n_rules = n;
    h.n_lin = uint32_t(lin.size());
    h.has_cls = img ? 1u : 0u;
    if (img) {
        const Cls4Image& im = *img;
        h.img_bytes = im.img_bytes; h.off_bounds = im.off_bounds; h.off_iclass = im.off_iclass;
        h.off_cells = im.off_cells; h.off_lists = im.off_lists; h.off_tmpl = im.off_tmpl;
        h.n_bounds = im.n_bounds; h.search_top = im.search_top; h.n_classes = im.n_classes;
        h.n_tmpl = im.n_tmpl; h.n_list_entries = im.n_list_entries; h.n_ctr = im.n_ctr;
        h.lds_bytes = im.lds_bytes;
        h.mode = im.mode;
        h.default_class = im.default_class;
        h.n_hash = im.n_hash;
        h.list_mode = im.list_mode;
        h.off_bv = im.off_bv;
        h.bv_steps_d = im.bv_steps_d;
        h.bv_steps_p = im.bv_steps_p;
        h.off_ptop = im.off_ptop;
        h.n_pclass = im.n_pclass;
        h.bv_wide = im.bv_wide;
        h.row_bytes = im.row_bytes;
        h.port_mul = im.port_mul;
        h.port_mask4 = im.port_mask4;
        h.port_dflt = im.port_dflt;
        h.default_row = im.default_row;
        h.n_hot = im.n_hot;
        h.off_hot = im.off_hot;
        h.n_lctr = im.n_lctr;
        h.ctr16 = im.ctr16;
        h.swap = im.swap;
        h.off_trie = im.off_trie;
        h.trie_depth = im.trie_depth;
        h.n_gcells = uint32_t(im.gcells.size());
        for (uint32_t i = 0; i < kMaxHashLens; ++i) {
            h.hash_mask[i] = im.hash_mask[i];
            h.hash_shift[i] = im.hash_shift[i];
            h.hash_cap[i] = im.hash_cap[i];
            h.hash_mul[i] = im.hash_mul[i];
            h.off_hash[i] = im.off_hash[i];
        }
    }
    auto al = [](uint64_t x) { return (x + 15) & ~uint64_t(15); };
    h.off_image = uint32_t(al(sizeof h + extra_bytes));
    h.off_ctr_rule = uint32_t(al(h.off_image + h.img_bytes));
    h.off_lin = uint32_t(al(h.off_ctr_rule + uint64_t(h.n_ctr) * 4));
    h.total_bytes = uint32_t(h.off_lin + lin.size() * sizeof(LinRule4));
    if (h.n_gcells) {
        h.off_gcells = uint32_t(al(h.total_bytes));
        h.total_bytes = h.off_gcells + h.n_gcells * 4u;
    }
    const uint32_t off_trailer = uint32_t(al(h.total_bytes));
    if (trailer) h.total_bytes = off_trailer + uint32_t(trailer->size() * 4);
    uint64_t need_o = 0;                      // the OTHER image: a nested blob (magic "CLSO")
    if (other) {
        write_blob(other, {}, n, 0x434C534Fu, nullptr, 0, nullptr, 0, &need_o);
        h.off_other = uint32_t(al(h.total_bytes));
        h.total_bytes = h.off_other + uint32_t(need_o);
    }
    *need = h.total_bytes;
    if (!blob || cap < h.total_bytes) return CLS_OK;
    uint8_t* b = static_cast<uint8_t*>(blob);
    std::memset(b, 0, h.total_bytes);
    std::memcpy(b, &h, sizeof h);
    if (extra_bytes) std::memcpy(b + sizeof h, extra, extra_bytes);
    if (trailer) {
        std::memcpy(b + sizeof h + trailer_field, &off_trailer, 4);   // extra header field: trailer offset
        std::memcpy(b + off_trailer, trailer->data(), trailer->size() * 4);
    }
    if (img) {
        std::memcpy(b + h.off_image, img->words.data(), img->img_bytes);
        std::memcpy(b + h.off_ctr_rule, img->ctr_rule.data(), size_t(h.n_ctr) * 4);
        if (h.n_gcells) std::memcpy(b + h.off_gcells, img->gcells.data(), size_t(h.n_gcells) * 4);
    }
    if (!lin.empty()) std::memcpy(b + h.off_lin, lin.data(), lin.size() * sizeof(LinRule4));
    if (other) write_blob(other, {}, n, 0x434C534Fu, nullptr, 0, b + h.off_other, need_o, &need_o);
    return CLS_OK;
}

int cls_gen_traffic_v16(cls_engine* e, const cls_traffic_spec16* sp, uint64_t first, uint64_t n,
                        uint8_t* src16, uint8_t* dst16, uint16_t* sport, uint16_t* dport, uint8_t* proto,
                        void* stream) {
    if (!e || !sp) return CLS_E_INVAL;
    std::lock_guard<std::mutex> g(e->mu);
    const DeviceGuard dg;        // the caller's device again on return
    return gen16_locked(e, sp, first, n, src16, dst16, sport, dport, proto, stream, true);
}

}  // extern "C"

int gen16_locked(cls_engine* e, const cls_traffic_spec16* sp, uint64_t first, uint64_t n, uint8_t* src16,
                 uint8_t* dst16, uint16_t* sport, uint16_t* dport, uint8_t* proto, void* stream, bool sync) {
    if ((src16 && !aligned(src16, 16)) || (dst16 && !aligned(dst16, 16)))
        return fail(e, CLS_E_INVAL, "src16/dst16 must be 16-byte aligned");
    HIPC(e, hipSetDevice(e->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : e->stream;
    // pools as (hi, lo) u64 pairs in address order
    auto pairs = [](const uint8_t* b, uint32_t m) {
        std::vector<uint64_t> v(size_t(m) * 2, 0);
        for (uint32_t j = 0; j < m; ++j)
            for (int k = 0; k < 16; ++k) v[2 * j + k / 8] = (v[2 * j + k / 8] << 8) | b[16 * size_t(j) + k];
        return v;
    };
    // the pairs live in the engine (an unsynchronised upload still reads
    // them after the call returns); an earlier such upload finishes first
    if (e->gen_pending) HIPC(e, hipStreamSynchronize(s));
    e->gen_pending = false;
    const std::vector<uint64_t> pods = pairs(sp->pod_ips, sp->n_pod_ips), dsta = pairs(sp->dst_addrs, sp->n_dst);
    std::vector<uint64_t>& hp = e->gen_pairs;
    hp.assign(pods.begin(), pods.end());
    hp.insert(hp.end(), dsta.begin(), dsta.end());
    const size_t bp = pods.size() * 8, bd = dsta.size() * 8, bl = sp->n_dst, bq = size_t(sp->n_ports) * 2;
    auto al = [](size_t x) { return (x + 15) & ~size_t(15); };
    HIPC(e, e->s_pool.ensure(al(bp) + al(bd) + al(bl) + al(bq) + 16));
    uint8_t* base = e->s_pool.as<uint8_t>();
    TrafficDev16 t;
    t.seed = sp->seed;
    t.pct_pod = sp->pct_pod_src; t.pct_dst = sp->pct_rule_dst;
    t.pct_port = sp->pct_table_port; t.pct_icmp = sp->pct_icmp;
    t.pods = reinterpret_cast<const uint64_t*>(base); t.n_pods = sp->n_pod_ips;
    t.dst_addrs = reinterpret_cast<const uint64_t*>(base + al(bp));
    t.dst_lens = base + al(bp) + al(bd); t.n_dst = sp->n_dst;
    t.ports = reinterpret_cast<const uint16_t*>(base + al(bp) + al(bd) + al(bl)); t.n_ports = sp->n_ports;
    if (bp) HIPC(e, hipMemcpyAsync(base, hp.data(), bp, hipMemcpyHostToDevice, s));
    if (bd) HIPC(e, hipMemcpyAsync(base + al(bp), hp.data() + pods.size(), bd, hipMemcpyHostToDevice, s));
    if (bl) HIPC(e, hipMemcpyAsync(base + al(bp) + al(bd), sp->dst_lens, bl, hipMemcpyHostToDevice, s));
    if (bq) HIPC(e, hipMemcpyAsync(base + al(bp) + al(bd) + al(bl), sp->ports, bq, hipMemcpyHostToDevice, s));
    e->gen_pending = !sync;
    HIPC(e, launch_gen16(t, first, n, reinterpret_cast<uint4*>(src16), reinterpret_cast<uint4*>(dst16), sport, dport,
                         proto, s));
    if (sync) HIPC(e, hipStreamSynchronize(s));   // the pools are engine scratch
    return CLS_OK;
}

extern "C" {

int cls_compile_v4(const cls_rule* rules, uint32_t n, void* blob, uint64_t cap, uint64_t* need,
                   const char* options) {
    if ((n && !rules) || !need) return CLS_E_INVAL;
    std::vector<SemRule> sem;
    std::string why;
    Opts o;
    if (!opts_parse(o, options, why)) return CLS_E_INVAL;
    const CompileScope scope(o);
    int rc = semantic_rules(rules, n, 4, sem, why);
    if (rc != CLS_OK) return rc;
    std::vector<LinRule4> lin = linear4(sem);
    Cls4Image img, oimg;
    const bool has = sem.size() > 8 && build_pair(sem, n, img, oimg, why);
    if (has && o.pair4) {
        // (option pair4: the connection pair launch's four-cell image, in the
        // main image's orientation, instead -- CPU tests of that compile)
        Cls4Image pimg;
        if (!build_pair4(sem, n, img.swap != 0, pimg, why)) return CLS_E_INVAL;
        return write_blob(&pimg, lin, n, 0x434C5334u, nullptr, 0, blob, cap, need, nullptr, 0, nullptr);
    }
    return write_blob(has ? &img : nullptr, lin, n, 0x434C5334u, nullptr, 0, blob, cap, need, nullptr, 0,
                      has ? &oimg : nullptr);
}


int cls_compile_v16(const cls_rule* rules, uint32_t n, void* blob, uint64_t cap, uint64_t* need,
                    const char* options) {
    if ((n && !rules) || !need) return CLS_E_INVAL;
    std::vector<SemRule> sem;
    std::string why;
    Opts o;
    if (!opts_parse(o, options, why)) return CLS_E_INVAL;
    const CompileScope scope(o);
    int rc = semantic_rules(rules, n, 0, sem, why);
    if (rc != CLS_OK) return rc;
    Cls16Image img;
    Cls4Image oimg;
    if (!build_cls16(sem, n, img, why) || !build_other4(img.sem, n, oimg, why)) return CLS_E_INVAL;
    if (o.pair4) {
        // (option pair4: the connection pair launch's four-cell image, in the
        // main image's orientation, instead; no OTHER image -- CPU tests of
        // that compile)
        Cls16Image pimg;
        if (!build_pair16(sem, n, img.core.swap != 0, pimg, why)) return CLS_E_INVAL;
        img = std::move(pimg);
    }
    cls_image_v16_header h16;
    std::memset(&h16, 0, sizeof h16);
    for (int sd = 0; sd < 2; ++sd) {
        h16.fe_key[sd] = img.fe_key[sd];
        h16.fe_val[sd] = img.fe_val[sd];
        h16.fe_top[sd] = img.fe_top[sd];
        h16.fe_n[sd] = img.fe_n[sd];
        h16.fe_k8[sd] = img.fe_k8[sd];
    }
    h16.src_mode = img.src_mode;
    h16.h4 = img.h4; h16.cap4 = img.cap4; h16.mul4 = img.mul4;
    h16.k6 = img.k6; h16.r6 = img.r6; h16.cap6 = img.cap6; h16.mul6 = img.mul6;
    for (int i = 0; i < 3; ++i) h16.fold[i] = img.fold[i];
    h16.dflt_row[0] = img.dflt_row[0];
    h16.dflt_row[1] = img.dflt_row[1];
    h16.src_search_val = img.src_search_val;
    h16.src_search_top = img.src_search_top;
    h16.src_search_k8 = img.src_search_k8;
    const size_t extra = sizeof h16 - sizeof h16.core;
    return write_blob(&img.core, linear4(img.sem), n, 0x434C3136u, reinterpret_cast<const uint8_t*>(&h16) + sizeof h16.core,
                      extra, blob, cap, need, img.src_mode >= 1 ? &img.src_search : nullptr,
                      offsetof(cls_image_v16_header, off_src_search) - sizeof h16.core, o.pair4 ? nullptr : &oimg);
}

}  // extern "C"
