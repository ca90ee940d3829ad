// The reachability matrix's kernels (kernels.hpp ReachTile; reach.cpp):
// reach_expand4 / reach_expand16 write a tile's connections as the arrays of
// a device connection batch, reach_reduce sums the tile's ConnectionActions
// into the per-probe histogram and the per-(probe, source) allow counts.
// Plain C++ throughout: vector stores, LDS and global atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "k_reach_dev.hpp"
#include "kernels.hpp"

namespace cls {

namespace {

template <bool K16>
__device__ __forceinline__ void reach_expand_body(const ReachTile& t, const ReachExpand& x) {
    using Addr = typename std::conditional<K16, uint4, uint32_t>::type;
    const Addr* ep = static_cast<const Addr*>(x.ep_addr);
    const uint32_t groups = (t.n + 3u) / 4u;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        const ReachCell c = reach_cell(t, 4u * g);
        ReachRow r = reach_row(t, c.row);
        uint32_t d = c.d;
        // the row's source and probe, reloaded when a carry moves the row
        uint32_t sif = x.ep_if[r.s];
        Addr sa = ep[r.s];
        uint2 pb = x.probe[t.p0 + r.p];
        uint32_t o_sif[4], o_dif[4], o_sp[4], o_dp[4], o_pr[4];
        Addr o_src[4], o_dst[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o_sif[k] = sif;
            o_dif[k] = x.ep_if[d];
            o_src[k] = sa;
            o_dst[k] = ep[d];
            o_sp[k] = pb.x & 0xFFFFu;
            o_dp[k] = pb.x >> 16;
            o_pr[k] = pb.y & 0xFFu;
            // the next cell: destination, then source, then probe -- only
            // while cells remain (the tile's last cell has no successor to
            // load: the rest of its group repeats it)
            if (k < 3 && 4u * g + k + 1u < t.n && ++d == t.n_ep) {
                d = 0;
                if (++r.s == t.n_ep) {
                    r.s = 0;
                    ++r.p;
                    pb = x.probe[t.p0 + r.p];
                }
                sif = x.ep_if[r.s];
                sa = ep[r.s];
            }
        }
        reinterpret_cast<uint4*>(x.src_if)[g] = uint4{o_sif[0], o_sif[1], o_sif[2], o_sif[3]};
        reinterpret_cast<uint4*>(x.dst_if)[g] = uint4{o_dif[0], o_dif[1], o_dif[2], o_dif[3]};
        if constexpr (K16) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                static_cast<uint4*>(x.src)[4u * g + k] = o_src[k];
                static_cast<uint4*>(x.dst)[4u * g + k] = o_dst[k];
            }
        } else {
            static_cast<uint4*>(x.src)[g] = uint4{o_src[0], o_src[1], o_src[2], o_src[3]};
            static_cast<uint4*>(x.dst)[g] = uint4{o_dst[0], o_dst[1], o_dst[2], o_dst[3]};
        }
        reinterpret_cast<uint2*>(x.sport)[g] = uint2{o_sp[0] | o_sp[1] << 16, o_sp[2] | o_sp[3] << 16};
        reinterpret_cast<uint2*>(x.dport)[g] = uint2{o_dp[0] | o_dp[1] << 16, o_dp[2] | o_dp[3] << 16};
        reinterpret_cast<uint32_t*>(x.proto)[g] = o_pr[0] | o_pr[1] << 8 | o_pr[2] << 16 | o_pr[3] << 24;
    }
}
__global__ __launch_bounds__(256) void reach_expand4(ReachTile t, ReachExpand x) { reach_expand_body<false>(t, x); }
__global__ __launch_bounds__(256) void reach_expand16(ReachTile t, ReachExpand x) { reach_expand_body<true>(t, x); }

__global__ __launch_bounds__(kReachBlock) void reach_reduce(ReachTile t, const uint8_t* verdict,
                                                            unsigned long long* hist, uint32_t* allow) {
    __shared__ uint32_t bins[4u * kReachLdsProbes];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t chunks = (t.n + kReachChunk - 1u) / kReachChunk;
    for (uint32_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const uint32_t c0 = ch * kReachChunk;                      // the chunk's first connection
        // the chunk's first probe: bins of probes [pb, pb + kReachLdsProbes) in LDS
        const uint32_t pb = reach_row(t, reach_cell(t, c0).row).p;
        if (threadIdx.x < 4u * kReachLdsProbes) bins[threadIdx.x] = 0u;
        __syncthreads();
        const uint32_t i0 = c0 + 4u * threadIdx.x;                 // the lane's four connections
        const uint32_t w0 = i0 - 4u * lane;                        // the wave's 256
        if (w0 < t.n) {                                            // wave-uniform
            const uint32_t wl = min(w0 + 255u, t.n - 1u);
            const uint32_t row_a = reach_cell(t, w0).row, row_b = reach_cell(t, wl).row;
            const uint32_t p_a = reach_row(t, row_a).p, p_b = reach_row(t, row_b).p;
            // the lane's verdict bytes (one 4-B load; the matrix's last,
            // partial group byte by byte: nothing is read past the tile)
            uint32_t v4 = 0u, live = 0u;
            if (i0 + 4u <= t.n) {
                v4 = *reinterpret_cast<const uint32_t*>(verdict + i0);
                live = 4u;
            } else if (i0 < t.n) {
                live = t.n - i0;
                for (uint32_t k = 0; k < live; ++k) v4 |= uint32_t(verdict[i0 + k]) << (8u * k);
            }
            // the lane's counts per ConnectionAction, u16 fields: actions 0, 1
            // in lo, 2 (CLS_CONN_ALLOW), 3 in hi
            uint32_t lo = 0u, hi = 0u;
            for (uint32_t k = 0; k < live; ++k) {
                const uint32_t v = (v4 >> (8u * k)) & 3u;
                if (v < 2u) lo += 1u << (16u * v);
                else hi += 1u << (16u * (v - 2u));
            }
            const bool one_probe = p_a == p_b, one_row = row_a == row_b;
            if (one_probe || one_row) {
                lo = wave_sum(lo);                                 // <= 256 per field
                hi = wave_sum(hi);
            }
            if (hist) {
                if (one_probe) {
                    if (lane < 4u) {
                        const uint32_t c = ((lane < 2u ? lo : hi) >> (16u * (lane & 1u))) & 0xFFFFu;
                        if (c) {
                            if (p_a - pb < kReachLdsProbes) atomicAdd(&bins[4u * (p_a - pb) + lane], c);
                            else atomicAdd(&hist[4ull * p_a + lane], (unsigned long long)c);
                        }
                    }
                } else {
                    ReachCell c = reach_cell(t, i0 < t.n ? i0 : w0);
                    ReachRow r = reach_row(t, c.row);
                    for (uint32_t k = 0; k < live; ++k) {
                        const uint32_t v = (v4 >> (8u * k)) & 3u;
                        if (r.p - pb < kReachLdsProbes) atomicAdd(&bins[4u * (r.p - pb) + v], 1u);
                        else atomicAdd(&hist[4ull * r.p + v], 1ull);
                        if (++c.d == t.n_ep) {
                            c.d = 0;
                            if (++r.s == t.n_ep) {
                                r.s = 0;
                                ++r.p;
                            }
                        }
                    }
                }
            }
            if (allow) {
                if (one_row) {
                    const uint32_t c = hi & 0xFFFFu;
                    if (lane == 0u && c) atomicAdd(&allow[row_a], c);
                } else {
                    // a wave across rows: each lane adds its cells' runs per row
                    ReachCell c = reach_cell(t, i0 < t.n ? i0 : w0);
                    uint32_t run = 0u;
                    for (uint32_t k = 0; k < live; ++k) {
                        run += ((v4 >> (8u * k)) & 3u) == 2u ? 1u : 0u;
                        if (++c.d == t.n_ep || k + 1u == live) {
                            if (run) atomicAdd(&allow[c.row], run);
                            run = 0u;
                            c.d = 0;
                            ++c.row;
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (hist && threadIdx.x < 4u * kReachLdsProbes && bins[threadIdx.x])
            atomicAdd(&hist[4ull * pb + threadIdx.x], (unsigned long long)bins[threadIdx.x]);
        __syncthreads();                                           // before the next chunk clears the bins
    }
}

}  // namespace

hipError_t launch_reach_expand(const ReachTile& t, const ReachExpand& x, bool k16, int n_cu, hipStream_t s) {
    if (!t.n) return hipSuccess;
    const int grid = reach_grid((uint64_t(t.n) + 3) / 4, 256, n_cu);
    if (k16) hipLaunchKernelGGL(reach_expand16, dim3(grid), dim3(256), 0, s, t, x);
    else hipLaunchKernelGGL(reach_expand4, dim3(grid), dim3(256), 0, s, t, x);
    return hipGetLastError();
}

hipError_t launch_reach_reduce(const ReachTile& t, const uint8_t* verdict, unsigned long long* hist,
                               uint32_t* allow, int n_cu, hipStream_t s) {
    if (!t.n || (!hist && !allow)) return hipSuccess;
    const int grid = reach_grid(t.n, kReachChunk, n_cu);
    hipLaunchKernelGGL(reach_reduce, dim3(grid), dim3(kReachBlock), 0, s, t, verdict, hist, allow);
    return hipGetLastError();
}

}  // namespace cls
