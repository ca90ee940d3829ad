// Connection batches, 16-byte layout: both tuples of every connection on the
// table's pair image in one launch (kernels.hpp launch_classify16_pair).
//
// The 16-byte twin of classify4_pair<..., kO4 = true> (k4_pair.hip).  The
// pair image (compile.hpp build_pair16) is the 16-byte image with a fourth
// cell per source class for protocols > 2, so every connection takes the main
// loop: no OTHER queue, no drain, no second image, and -- unlike the slot
// launches it replaces -- no global source table (src_mode 1 and 2 yield class
// rows for every protocol; src_mode 0 takes the rep through the core's own
// source lookup to a row with four cells).  One launch stages the image once
// per workgroup (the u16 slot -> rule map beside it when the batch counts),
// reads each connection's fields once (37 B) and writes one result byte, or
// one or two counter-index words, per connection; two slot launches staged
// the image twice, read 2 x 35 B and wrote 8 B.
//
// Both 16-byte addresses of a connection go through both sides of the front
// end: the SYN tuple is (side0(s), side1(d), dport), the SYN-ACK tuple
// (side0(d), side1(s), sport).  A destination-keyed image exchanges the
// roles; the host passes src and dst exchanged (as classify4_pair's frame).
//
// Connection order: wave-contiguous, as classify16_cls.  A wave's step
// covers 64 x kPair16Conns consecutive connections and lane l takes base +
// 64 k + l, so each 16-B address load instruction reads 1 KiB contiguous per
// wave and the port, protocol and result accesses are contiguous per
// instruction too (the lane-owns-four-consecutive order strides 64 B per lane
// and over-fetched 25 % of the algorithmic bytes on the 16-byte classify
// stream, profiles/r01_pmc_config5_lane4order.json).  The next step's fields
// are fetched before this step's lookups, the first step's before the image
// staging (as classify4_pair: a batch of a few Mi connections gives each lane
// only a few steps).
//
// Registers: a connection is two chains of dependent LDS reads over four
// 16-byte front-end lookups, about twice an IPv4 pair's state, and the
// prefetch holds a step's fields (11 VGPRs per connection) twice.  Two
// connections per lane per step, classified together (four chains
// interleaved) or -- with the host-route hashes, whose probes hold 16-B keys
// -- one at a time, keep every variant within the 128 VGPRs of a 1024-thread
// workgroup without scratch: 82-84 VGPRs behind the interval search, 94-96
// behind the trie, 97-99 behind the hashes.  Two connections together behind
// the hashes spill (128 VGPRs, 68 B of scratch); their front ends one after
// the other and the four chains together fit at 127-128 VGPRs and measured
// 52.8 against 54.1 us on config 5 at 4 Mi connections -- not kept.
#include "kernels_dev.hpp"

namespace cls {

namespace {

static_assert(kClsBlock == kPairBlock, "launch_classify16_pair's grid is sized for this block");

// kFe: the source-side front end -- 0 interval search -> rep, then the
// core's own source lookup (kMode 0, 1, 2, 4); 1 host-route hashes, 2 IPv4
// trie / non-IPv4 search -> class row (kMode 3)
template <int kMode, int kList, int kFe>
__global__ __launch_bounds__(kClsBlock) void classify16_pair(Cls4Dev t, Fe16 fe, Pkts16 p, const uint16_t* sport,
                                                             uint32_t* out, uint64_t stride,
                                                             const uint32_t* slot_rule, uint32_t ctr_base,
                                                             uint32_t wbytes, const uint16_t* slot16, uint32_t srl,
                                                             uint32_t srl_n) {
    extern __shared__ uint4 smem[];
    constexpr int C = int(kPair16Conns);
    constexpr int G = kFe == 1 ? 1 : 2;                   // connections classified together
    static_assert(C % G == 0, "a step is whole groups");
    const uint32_t nthreads = gridDim.x * blockDim.x;
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    // whole wave-steps only (wave-uniform trip counts); the rest is the tail's
    const uint32_t nsteps = uint32_t(p.n / (64u * C)) * 64u;
    struct Fields {
        uint4 s[C], d[C];
        uint32_t dp[C], sp[C], pr[C];
    };
    // lane-step g -> its first connection; the others follow at + 64 k
    auto first = [](uint32_t g) { return uint32_t(C) * (g & ~63u) + (g & 63u); };
    auto fetch = [&](uint32_t g, Fields& f) {
        const uint32_t base = first(g);
#pragma unroll
        for (int k = 0; k < C; ++k) {
            f.s[k] = ldnt(at(p.src, base + 64u * k));
            f.d[k] = ldnt(at(p.dst, base + 64u * k));
        }
#pragma unroll
        for (int k = 0; k < C; ++k) {
            f.dp[k] = __builtin_nontemporal_load(p.dport + base + 64u * k);
            f.sp[k] = __builtin_nontemporal_load(sport + base + 64u * k);
            f.pr[k] = __builtin_nontemporal_load(p.proto + base + 64u * k);
        }
    };
    Fields nx{};
    if (tid < nsteps) fetch(tid, nx);
    // the image and (counting) the slot -> rule map as u16 at LDS byte srl
    // (srl_n 16-B units) in one round of loads
    lds_copy2(smem, reinterpret_cast<const uint4*>(t.img), t.img_bytes / 16u, srl / 16u,
              reinterpret_cast<const uint4*>(slot16), srl ? srl_n : 0u);
    __syncthreads();
    const Img<true> im{nullptr};
    // a word's payload: the slot, or (counting) its counter index (from the
    // LDS copy of the map when there is one)
    auto key = [&](uint32_t slot) {
        return srl ? ctr_base + *lds16_t(srl + 2u * slot) : slot_rule ? ctr_base + slot_rule[slot] : slot;
    };
    // one connection's two words: u32, u16 (wbytes 2: the host keeps the
    // counter indices below 2^14; both in one u32), or (wbytes 1) its two
    // results in one byte
    auto put = [&](uint32_t i, uint32_t w0, uint32_t w1) {
        if (wbytes == 1u) {
            reinterpret_cast<uint8_t*>(out)[i] = uint8_t((w0 & 3u) | (w1 & 3u) << 2);
        } else if (wbytes == 2u) {
            out[i] = (w0 & 0xFFFFu) | w1 << 16;
        } else {
            out[i] = w0;
            out[stride + i] = w1;
        }
    };
    // Both tuples of N connections: the 2 N addresses through both sides of
    // the front end, then the 2 N chains of the core interleaved.
    auto pairs = [&](const auto& s16, const auto& d16, const auto& dp, const auto& sp, const auto& pr, auto& w0,
                     auto& w1) {
        constexpr int N = int(sizeof(w0) / 4);
        uint4 a[2 * N];
#pragma unroll
        for (int q = 0; q < N; ++q) {
            a[q] = s16[q];
            a[N + q] = d16[q];
        }
        uint32_t r0[2 * N], r1[2 * N];                    // source side (rep or row), destination side (rep)
        if constexpr (kFe == 1) src_hash16(im, fe, a, r0);
        else if constexpr (kFe == 2) src_trie16(im, t, fe, a, r0);
        else fe_rep(im, fe.key[0], fe.val[0], fe.top[0], fe.k8[0], a, r0);
        fe_rep(im, fe.key[1], fe.val[1], fe.top[1], fe.k8[1], a, r1);
        uint32_t S[2 * N], D[2 * N], P[2 * N], R[2 * N], rv[2 * N], k[2 * N];
#pragma unroll
        for (int q = 0; q < N; ++q) {
            S[q] = r0[q]; S[N + q] = r0[N + q];           // SYN: the source's; SYN-ACK: the destination's
            D[q] = r1[N + q]; D[N + q] = r1[q];
            P[q] = dp[q]; P[N + q] = sp[q];
            R[q] = pr[q]; R[N + q] = pr[q];
        }
        classify_n<2 * N, true, kMode, kList, -1, 4>(im, t, S, D, P, R, rv, k);
#pragma unroll
        for (int q = 0; q < N; ++q) {
            w0[q] = rv[q] | (key(k[q]) << 2);
            w1[q] = rv[N + q] | (key(k[N + q]) << 2);
        }
    };
    for (uint32_t g = tid; g < nsteps; g += nthreads) {
        const Fields f = nx;
        if (g + nthreads < nsteps) fetch(g + nthreads, nx);
        const uint32_t base = first(g);
#pragma unroll
        for (int h = 0; h < C / G; ++h) {
            uint4 sg[G], dg[G];
            uint32_t dpg[G], spg[G], prg[G], w0[G], w1[G];
#pragma unroll
            for (int q = 0; q < G; ++q) {
                sg[q] = f.s[G * h + q];
                dg[q] = f.d[G * h + q];
                dpg[q] = f.dp[G * h + q];
                spg[q] = f.sp[G * h + q];
                prg[q] = f.pr[G * h + q];
            }
            pairs(sg, dg, dpg, spg, prg, w0, w1);
#pragma unroll
            for (int q = 0; q < G; ++q) put(base + 64u * (G * h + q), w0[q], w1[q]);
        }
    }
    // the rest, one connection per lane: the same lookups, the same words
    for (uint32_t i = nsteps * uint32_t(C) + tid; i < uint32_t(p.n); i += nthreads) {
        const uint4 s1[1] = {ldnt(at(p.src, i))}, d1[1] = {ldnt(at(p.dst, i))};
        const uint32_t dp1[1] = {p.dport[i]}, sp1[1] = {sport[i]}, pr1[1] = {p.proto[i]};
        uint32_t w0[1], w1[1];
        pairs(s1, d1, dp1, sp1, pr1, w0, w1);
        put(i, w0[0], w1[0]);
    }
}

template <int kMode, int kList, int kFe>
void launch_pair16(const Cls4Dev& t, const Fe16& fe, const Pkts16& p, const uint16_t* sport, uint32_t* out,
                   uint64_t stride, const uint32_t* slot_rule, uint32_t ctr_base, uint32_t wbytes, const PairMap& sm,
                   const LaunchCfg& cfg) {
    const size_t lds = (sm.srl ? size_t(sm.srl) + 16u * sm.n16 : (size_t(t.img_bytes) + 15u) & ~size_t(15)) + 16u;
    lds_attr<classify16_pair<kMode, kList, kFe>>();
    hipLaunchKernelGGL((classify16_pair<kMode, kList, kFe>), dim3(cfg.grid), dim3(kClsBlock), lds, cfg.stream, t, fe,
                       p, sport, out, stride, slot_rule, ctr_base, wbytes, sm.map, sm.srl, sm.n16);
}

}  // namespace

hipError_t launch_classify16_pair(const Cls4Dev& t, const Fe16& fe, const Pkts16& p, const uint16_t* sport,
                                  uint32_t* out, uint64_t stride, const uint32_t* slot_rule, uint32_t ctr_base,
                                  uint32_t wbytes, const PairMap& sm, const LaunchCfg& cfg) {
    if (!pair16_kernel_exists(t.mode, t.list_mode, fe.src_mode) || t.gcells) return hipErrorInvalidValue;
    // the core's source lookup (kernels_dev.hpp src_variant; 3: rows from the front end)
    const int src = fe.src_mode ? 4 : src_variant(t);
    const int kfe = int(fe.src_mode);
#define PAIR16_CASE(S, M, L, F) \
    case 8 * S + L: \
        if (kfe == F) launch_pair16<M, L, F>(t, fe, p, sport, out, stride, slot_rule, ctr_base, wbytes, sm, cfg); \
        else return hipErrorInvalidValue; \
        break;
#define PAIR16_ROWS(L) \
    case 8 * 4 + L: \
        if (kfe == 1) launch_pair16<3, L, 1>(t, fe, p, sport, out, stride, slot_rule, ctr_base, wbytes, sm, cfg); \
        else launch_pair16<3, L, 2>(t, fe, p, sport, out, stride, slot_rule, ctr_base, wbytes, sm, cfg); \
        break;
    switch (8 * src + int(t.list_mode)) {
        PAIR16_CASE(0, 0, 0, 0) PAIR16_CASE(0, 0, 1, 0) PAIR16_CASE(0, 0, 2, 0) PAIR16_CASE(0, 0, 3, 0)
        PAIR16_CASE(0, 0, 4, 0)
        PAIR16_CASE(1, 1, 0, 0) PAIR16_CASE(1, 1, 1, 0) PAIR16_CASE(1, 1, 2, 0) PAIR16_CASE(1, 1, 3, 0)
        PAIR16_CASE(1, 1, 4, 0)
        PAIR16_CASE(2, 2, 0, 0) PAIR16_CASE(2, 2, 1, 0) PAIR16_CASE(2, 2, 2, 0) PAIR16_CASE(2, 2, 3, 0)
        PAIR16_CASE(2, 2, 4, 0)
        PAIR16_CASE(3, 4, 3, 0) PAIR16_CASE(3, 4, 4, 0)
        PAIR16_ROWS(0) PAIR16_ROWS(1) PAIR16_ROWS(2) PAIR16_ROWS(3) PAIR16_ROWS(4)
    default: return hipErrorInvalidValue;
    }
#undef PAIR16_CASE
#undef PAIR16_ROWS
    return hipGetLastError();
}

}  // namespace cls
