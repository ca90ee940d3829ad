// Host race check (ThreadSanitizer) of the rule compiler (vpp_amd/csrc
// compile.cpp, options.cpp): the part of the library's threading contract
// that runs without a GPU.  cls_table_put and cls_acl_put compile outside any
// process-wide lock -- two engines compile at once, each under the options of
// its own compile (options.hpp CompileScope, a thread-local) -- so the
// compiler must share nothing writable between threads.
//
// Eight threads compile different ACLs of tools/asan/dump_acls.py at once,
// each thread under another CompileScope (trie / orient / wide combined):
// semantic_rules, build_cls4, build_other4, build_pair4, build_cls16,
// build_pair16.  Every image's words are then compared with a single-threaded
// pass over the same (ACL, options) pairs.  Exit status 1 on a difference;
// tools/tsan/run.sh makes a TSan report exit 1 too.  CPU only.
// build + run: tools/tsan/run.sh
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../vpp_amd/csrc/compile.hpp"

using namespace cls;

namespace {

constexpr int kThreads = 8;
constexpr size_t kAcls = 48;       // the random ACLs of both families (5 .. 600 rules)

struct Acl {
    std::vector<cls_rule> rules;
    std::vector<std::string> nets;     // 2 per rule; "-" = NULL
    void bind() {
        for (size_t i = 0; i < rules.size(); ++i) {
            rules[i].src_network = nets[2 * i] == "-" ? nullptr : nets[2 * i].c_str();
            rules[i].dst_network = nets[2 * i + 1] == "-" ? nullptr : nets[2 * i + 1].c_str();
        }
    }
};

bool read_acls(const char* path, std::vector<Acl>& out) {
    FILE* f = std::fopen(path, "r");
    if (!f) return false;
    char line[4096];
    Acl cur;
    while (std::fgets(line, sizeof line, f)) {
        if (line[0] == '=') {
            out.push_back(std::move(cur));
            cur = Acl();
            continue;
        }
        cls_rule r;
        std::memset(&r, 0, sizeof r);
        char src[256], dst[256];
        unsigned v[13];
        int act;
        if (std::sscanf(line, "%u %d %255s %255s %u %u %u %u %u %u %u %u %u %u %u %u", &v[0], &act, src, dst, &v[1],
                        &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9], &v[10], &v[11], &v[12]) != 16) {
            std::fclose(f);
            return false;
        }
        r.flags = v[0];
        r.acl_action = act;
        r.tcp_src_lo = v[1]; r.tcp_src_hi = v[2]; r.tcp_dst_lo = v[3]; r.tcp_dst_hi = v[4];
        r.udp_src_lo = v[5]; r.udp_src_hi = v[6]; r.udp_dst_lo = v[7]; r.udp_dst_hi = v[8];
        r.icmp_code_first = v[9]; r.icmp_code_last = v[10]; r.icmp_type_first = v[11]; r.icmp_type_last = v[12];
        cur.rules.push_back(r);
        cur.nets.push_back(src);
        cur.nets.push_back(dst);
    }
    std::fclose(f);
    for (auto& a : out) a.bind();       // the strings' storage is stable now
    return true;
}

// the options of thread t: every thread another combination
Opts opts_of(int t) {
    static const int trie[kThreads] = {-1, 0, 1, -1, 0, 1, -1, 0};
    static const int orient[kThreads] = {-1, 0, 1, 1, -1, 0, 0, 1};
    static const int wide[kThreads] = {-1, -1, -1, 0, 0, 0, 1, 1};
    Opts o;
    o.trie = trie[t];
    o.orient = orient[t];
    o.wide = wide[t];
    return o;
}

void put(std::vector<uint32_t>& d, const Cls4Image& img, bool ok) {
    d.push_back(ok ? 0x600Du : 0xBADu);
    if (!ok) return;
    d.push_back(uint32_t(img.words.size()));
    d.insert(d.end(), img.words.begin(), img.words.end());
    d.push_back(uint32_t(img.gcells.size()));
    d.insert(d.end(), img.gcells.begin(), img.gcells.end());
    d.push_back(uint32_t(img.ctr_rule.size()));
    d.insert(d.end(), img.ctr_rule.begin(), img.ctr_rule.end());
    for (uint32_t x : {img.mode, img.list_mode, img.swap, img.lds_bytes, img.n_lctr, img.ctr16, img.n_hot}) d.push_back(x);
}

void put16(std::vector<uint32_t>& d, const Cls16Image& img, bool ok) {
    put(d, img.core, ok);
    if (!ok) return;
    d.push_back(img.src_mode);
    d.push_back(uint32_t(img.src_search.size()));
    d.insert(d.end(), img.src_search.begin(), img.src_search.end());
}

// Everything the compiler makes of one ACL under `o`, as words.
std::vector<uint32_t> compile_all(const Acl& a, const Opts& o) {
    std::vector<uint32_t> d;
    const CompileScope scope(o);
    const uint32_t n = uint32_t(a.rules.size());
    std::string why;
    std::vector<SemRule> sem;
    const int rc4 = semantic_rules(a.rules.data(), n, 4, sem, why);
    d.push_back(uint32_t(rc4));
    if (rc4 == CLS_OK && sem.size() > 8) {
        Cls4Image img, oimg, pimg;
        const bool ok = build_cls4(sem, n, img, why);
        put(d, img, ok);
        if (ok) {
            put(d, oimg, build_other4(img.swap ? swap_sides(sem) : sem, n, oimg, why));
            put(d, pimg, build_pair4(sem, n, img.swap != 0, pimg, why));
        }
    }
    std::vector<SemRule> s16;
    const int rc16 = semantic_rules(a.rules.data(), n, 0, s16, why);
    d.push_back(uint32_t(rc16));
    if (rc16 == CLS_OK) {
        Cls16Image img, pimg;
        const bool ok = build_cls16(s16, n, img, why);
        put16(d, img, ok);
        if (ok) {
            Cls4Image oimg;
            put(d, oimg, build_other4(img.sem, n, oimg, why));
            put16(d, pimg, build_pair16(s16, n, img.core.swap != 0, pimg, why));
        }
    }
    return d;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::vector<Acl> acls;
    if (!read_acls(argv[1], acls) || acls.empty()) return 2;
    if (acls.size() > kAcls) acls.resize(kAcls);
    for (auto& a : acls) a.bind();                  // (resize may have moved them)
    const size_t n = acls.size();
    // ACL i is thread i % kThreads's, in both passes
    std::vector<std::vector<uint32_t>> par(n), seq(n);
    std::vector<std::thread> th;
    for (int t = 0; t < kThreads; ++t)
        th.emplace_back([&, t] {
            const Opts o = opts_of(t);
            for (size_t i = size_t(t); i < n; i += kThreads) par[i] = compile_all(acls[i], o);
        });
    for (auto& x : th) x.join();
    for (size_t i = 0; i < n; ++i) seq[i] = compile_all(acls[i], opts_of(int(i % kThreads)));
    int diffs = 0, images = 0;
    size_t words = 0;
    for (size_t i = 0; i < n; ++i) {
        if (par[i] != seq[i]) {
            std::printf("acl %zu (%zu rules, thread %zu): %zu words concurrently, %zu alone, or other words\n", i,
                        acls[i].rules.size(), i % kThreads, par[i].size(), seq[i].size());
            ++diffs;
        }
        for (uint32_t w : seq[i]) images += w == 0x600Du;   // (a count for the log line; an image word may look alike)
        words += seq[i].size();
    }
    std::printf("%zu ACLs on %d threads, about %d images, %zu words compared, %d differences\n", n, kThreads, images,
                words, diffs);
    return diffs ? 1 : 0;
}
