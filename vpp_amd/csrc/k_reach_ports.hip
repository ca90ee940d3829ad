// The reachability port sweep's kernels (kernels.hpp ReachPortsTile;
// reach.cpp cls_reach_ports).  reach_ports_expand4 / reach_ports_expand16
// write a tile's rows -- every pair x one representative port per class -- as
// the arrays of a device connection batch; reach_ports_count counts the rows
// that start a range per chunk and sums the pairs' runs, their ALLOW ports
// and the histogram, each row weighted by its class's width;
// reach_ports_emit, behind reach_diff_scan of the chunk counts, writes the
// run-length records.  Plain C++ throughout: vector stores, LDS and global
// atomics.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "k_reach_dev.hpp"
#include "kernels.hpp"

namespace cls {

namespace {

constexpr uint32_t kWaves = kReachBlock / 64u;

// Row i of the tile: its pair after the tile's first, that pair's endpoints,
// its class.  Two 32-bit divisions per lane; the lane's following rows advance
// by carries.
struct PortsRow {
    uint32_t pair, s, d, k;
};
__device__ __forceinline__ PortsRow ports_row(const ReachPortsTile& t, uint32_t i) {
    PortsRow r;
    r.pair = i / t.K;
    r.k = i - r.pair * t.K;
    const uint32_t x = t.d0 + r.pair;            // < 2^18 + 2^30
    const uint32_t row = x / t.n_ep;
    r.d = x - row * t.n_ep;
    r.s = t.s0 + row;
    return r;
}
__device__ __forceinline__ void ports_next(const ReachPortsTile& t, PortsRow& r) {
    if (++r.k == t.K) {
        r.k = 0;
        ++r.pair;
        if (++r.d == t.n_ep) {
            r.d = 0;
            ++r.s;
        }
    }
}
// ports of class k
__device__ __forceinline__ uint32_t ports_width(const ReachPortsTile& t, uint32_t k) {
    return (k + 1u < t.K ? uint32_t(t.lo[k + 1u]) : 65536u) - uint32_t(t.lo[k]);
}

template <bool K16>
__device__ __forceinline__ void ports_expand_body(const ReachPortsTile& t, const ReachPortsExpand& x) {
    using Addr = typename std::conditional<K16, uint4, uint32_t>::type;
    const Addr* ep = static_cast<const Addr*>(x.ep_addr);
    const uint32_t groups = (t.n + 3u) / 4u;
    const uint32_t sp2 = x.sport | x.sport << 16, pr4 = x.proto * 0x01010101u;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        PortsRow r = ports_row(t, 4u * g);
        // the pair's endpoints, reloaded when a carry moves the pair
        uint32_t sif = x.ep_if[r.s], dif = x.ep_if[r.d];
        Addr sa = ep[r.s], da = ep[r.d];
        uint32_t o_sif[4], o_dif[4], o_dp[4];
        Addr o_src[4], o_dst[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o_sif[j] = sif;
            o_dif[j] = dif;
            o_src[j] = sa;
            o_dst[j] = da;
            o_dp[j] = t.lo[r.k];
            // the next row -- only while rows remain (the tile's last row has
            // no successor to load: the rest of its group repeats it)
            if (j < 3 && 4u * g + j + 1u < t.n) {
                const uint32_t was = r.pair;
                ports_next(t, r);
                if (r.pair != was) {
                    sif = x.ep_if[r.s];
                    dif = x.ep_if[r.d];
                    sa = ep[r.s];
                    da = ep[r.d];
                }
            }
        }
        reinterpret_cast<uint4*>(x.src_if)[g] = uint4{o_sif[0], o_sif[1], o_sif[2], o_sif[3]};
        reinterpret_cast<uint4*>(x.dst_if)[g] = uint4{o_dif[0], o_dif[1], o_dif[2], o_dif[3]};
        if constexpr (K16) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                static_cast<uint4*>(x.src)[4u * g + j] = o_src[j];
                static_cast<uint4*>(x.dst)[4u * g + j] = o_dst[j];
            }
        } else {
            static_cast<uint4*>(x.src)[g] = uint4{o_src[0], o_src[1], o_src[2], o_src[3]};
            static_cast<uint4*>(x.dst)[g] = uint4{o_dst[0], o_dst[1], o_dst[2], o_dst[3]};
        }
        reinterpret_cast<uint2*>(x.sport_out)[g] = uint2{sp2, sp2};
        reinterpret_cast<uint2*>(x.dport_out)[g] = uint2{o_dp[0] | o_dp[1] << 16, o_dp[2] | o_dp[3] << 16};
        reinterpret_cast<uint32_t*>(x.proto_out)[g] = pr4;
    }
}
__global__ __launch_bounds__(256) void reach_ports_expand4(ReachPortsTile t, ReachPortsExpand x) {
    ports_expand_body<false>(t, x);
}
__global__ __launch_bounds__(256) void reach_ports_expand16(ReachPortsTile t, ReachPortsExpand x) {
    ports_expand_body<true>(t, x);
}

// The lane's four verdict bytes (one 4-B load; the tile's last, partial group
// byte by byte: nothing is read past the tile) and the byte of the row before
// them (unused at row 0, which starts a pair).
struct PortsWords {
    uint32_t v4, live, prev;
};
__device__ __forceinline__ PortsWords ports_load(const ReachPortsTile& t, const uint8_t* verdict, uint32_t i0) {
    PortsWords w{0u, 0u, 0u};
    if (i0 + 4u <= t.n) {
        w.v4 = *reinterpret_cast<const uint32_t*>(verdict + i0);
        w.live = 4u;
    } else if (i0 < t.n) {
        w.live = t.n - i0;
        for (uint32_t j = 0; j < w.live; ++j) w.v4 |= uint32_t(verdict[i0 + j]) << (8u * j);
    }
    if (w.live && i0) w.prev = verdict[i0 - 1u];
    return w;
}
__device__ __forceinline__ uint32_t byte_of(uint32_t w, uint32_t j) { return (w >> (8u * j)) & 0xFFu; }

__global__ __launch_bounds__(kReachBlock) void reach_ports_count(ReachPortsTile t, const uint8_t* verdict,
                                                                 uint32_t* chunk_count, uint32_t* runs,
                                                                 uint32_t* allow, unsigned long long* hist) {
    __shared__ uint32_t bins[4];                                   // <= kReachChunk x 65536 per chunk
    __shared__ uint32_t n_starts;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t chunks = (t.n + kReachChunk - 1u) / kReachChunk;
    for (uint32_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        if (threadIdx.x < 4u) bins[threadIdx.x] = 0u;
        if (threadIdx.x == 4u) n_starts = 0u;
        __syncthreads();
        const uint32_t i0 = ch * kReachChunk + 4u * threadIdx.x;   // the lane's four rows
        const uint32_t w0 = i0 - 4u * lane;                        // the wave's 256
        if (w0 < t.n) {                                            // wave-uniform
            const PortsWords w = ports_load(t, verdict, i0);
            PortsRow r = ports_row(t, i0 < t.n ? i0 : w0);
            uint32_t h[4] = {0u, 0u, 0u, 0u};                      // <= 4 x 65536 each
            uint32_t starts = 0u, run = 0u, ok = 0u, prev = w.prev;
            for (uint32_t j = 0; j < w.live; ++j) {
                const uint32_t v = byte_of(w.v4, j), width = ports_width(t, r.k);
                const uint32_t st = (r.k == 0u || v != prev) ? 1u : 0u;
                prev = v;
                starts += st;
                run += st;
#pragma unroll
                for (uint32_t a = 0; a < 4u; ++a) h[a] += (v & 3u) == a ? width : 0u;
                ok += v == 2u ? width : 0u;                        // CLS_CONN_ALLOW
                // the lane's sums of one pair, added when its rows leave the pair
                const uint32_t pair = r.pair;
                ports_next(t, r);
                if (r.pair != pair || j + 1u == w.live) {
                    if (runs && run) atomicAdd(&runs[pair], run);
                    if (allow && ok) atomicAdd(&allow[pair], ok);
                    run = 0u;
                    ok = 0u;
                }
            }
            if (chunk_count) {
                starts = wave_sum(starts);
                if (lane == 0u && starts) atomicAdd(&n_starts, starts);
            }
            if (hist) {
#pragma unroll
                for (uint32_t a = 0; a < 4u; ++a) h[a] = wave_sum(h[a]);   // <= 256 x 65536
                if (lane < 4u) {
                    const uint32_t c = lane == 0u ? h[0] : lane == 1u ? h[1] : lane == 2u ? h[2] : h[3];
                    if (c) atomicAdd(&bins[lane], c);
                }
            }
        }
        __syncthreads();
        if (hist && threadIdx.x < 4u && bins[threadIdx.x])
            atomicAdd(&hist[threadIdx.x], (unsigned long long)bins[threadIdx.x]);
        if (chunk_count && threadIdx.x == 4u) chunk_count[ch] = n_starts;
        __syncthreads();                                           // before the next chunk clears them
    }
}

__global__ __launch_bounds__(kReachBlock) void reach_ports_emit(ReachPortsTile t, const uint8_t* verdict,
                                                                const unsigned long long* chunk_base, uint4* ranges,
                                                                unsigned long long cap) {
    __shared__ uint32_t wave_n[kWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t chunks = (t.n + kReachChunk - 1u) / kReachChunk;
    for (uint32_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        // workgroup-uniform: the chunk's starts have indices from first on,
        // the range that reaches into it has first - 1 -- all past cap
        const unsigned long long first = chunk_base[ch];
        if (first > cap) continue;
        const uint32_t i0 = ch * kReachChunk + 4u * threadIdx.x;   // the lane's four rows
        const PortsWords w = ports_load(t, verdict, i0);
        PortsRow r = ports_row(t, i0 < t.n ? i0 : 0u);
        // the lane's starts (bit j: row i0 + j starts a range)
        uint32_t st = 0u, prev = w.prev, k = r.k;
        for (uint32_t j = 0; j < w.live; ++j) {
            const uint32_t v = byte_of(w.v4, j);
            if (k == 0u || v != prev) st |= 1u << j;
            prev = v;
            if (++k == t.K) k = 0u;
        }
        // the starts before the lane's in its wave (row order: the lower
        // lanes' rows come first), and the wave's
        uint32_t below = 0u, mine = 0u;
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const unsigned long long m = __ballot((st >> j) & 1u);
            below += __popcll(m & ((1ull << lane) - 1ull));
            mine += __popcll(m);
        }
        if (lane == 0u) wave_n[wave] = mine;
        __syncthreads();
        unsigned long long at = first + below;                     // the index of the lane's next start
        for (uint32_t j = 0; j < wave; ++j) at += wave_n[j];
        // the byte behind the lane's rows (read only where a row follows
        // inside the pair: the tile ends with a pair)
        const uint32_t after = w.live && i0 + w.live < t.n ? uint32_t(verdict[i0 + w.live]) : 0u;
        for (uint32_t j = 0; j < w.live; ++j) {
            const uint32_t v = byte_of(w.v4, j);
            const bool start = (st >> j) & 1u;
            const uint32_t next = j + 1u < w.live ? byte_of(w.v4, j + 1u) : after;
            const bool last = r.k + 1u == t.K;
            const bool end = last || next != v;
            const uint32_t hi = last ? 65535u : uint32_t(t.lo[r.k + 1u]) - 1u;
            if (start) {
                if (at < cap) {
                    const uint32_t lo = t.lo[r.k];
                    if (end) {
                        ranges[at] = uint4{r.s, r.d, lo | hi << 16, v};
                    } else {
                        // (port_hi is the end row's: the two write disjoint bytes)
                        uint32_t* rec = reinterpret_cast<uint32_t*>(ranges + at);
                        *reinterpret_cast<uint2*>(rec) = uint2{r.s, r.d};
                        *reinterpret_cast<uint16_t*>(rec + 2) = uint16_t(lo);
                        rec[3] = v;
                    }
                }
                ++at;
            }
            // at >= 1 here: the tile's first row is a start
            if (end && !start && at - 1ull < cap)
                reinterpret_cast<uint16_t*>(ranges + (at - 1ull))[5] = uint16_t(hi);
            ports_next(t, r);
        }
        __syncthreads();                                           // before the next chunk's wave counts
    }
}

}  // namespace

hipError_t launch_reach_ports_expand(const ReachPortsTile& t, const ReachPortsExpand& x, bool k16, int n_cu,
                                     hipStream_t s) {
    if (!t.n) return hipSuccess;
    const int grid = reach_grid((uint64_t(t.n) + 3) / 4, 256, n_cu);
    if (k16) hipLaunchKernelGGL(reach_ports_expand16, dim3(grid), dim3(256), 0, s, t, x);
    else hipLaunchKernelGGL(reach_ports_expand4, dim3(grid), dim3(256), 0, s, t, x);
    return hipGetLastError();
}

hipError_t launch_reach_ports_count(const ReachPortsTile& t, const uint8_t* verdict, uint32_t* chunk_count,
                                    uint32_t* runs, uint32_t* allow, unsigned long long* hist, int n_cu,
                                    hipStream_t s) {
    if (!t.n || (!chunk_count && !runs && !allow && !hist)) return hipSuccess;
    const int grid = reach_grid(t.n, kReachChunk, n_cu);
    hipLaunchKernelGGL(reach_ports_count, dim3(grid), dim3(kReachBlock), 0, s, t, verdict, chunk_count, runs, allow,
                       hist);
    return hipGetLastError();
}

hipError_t launch_reach_ports_emit(const ReachPortsTile& t, const uint8_t* verdict,
                                   const unsigned long long* chunk_base, uint4* ranges, unsigned long long cap,
                                   int n_cu, hipStream_t s) {
    if (!t.n || !ranges || !cap) return hipSuccess;
    const int grid = reach_grid(t.n, kReachChunk, n_cu);
    hipLaunchKernelGGL(reach_ports_emit, dim3(grid), dim3(kReachBlock), 0, s, t, verdict, chunk_base, ranges, cap);
    return hipGetLastError();
}

}  // namespace cls
