// The external sweep's kernels (kernels.hpp ReachExtTile; reach.cpp
// cls_reach_external).  reach_ext_expand4 / reach_ext_expand16 write a tile's
// rows -- every (direction, probe, endpoint) line x one representative remote
// address per class -- as the arrays of a device connection batch;
// reach_ext_count counts the rows that start a range per chunk and sums the
// lines' runs, their ALLOW addresses and the histogram per (direction, probe),
// each row weighted by its class's width; reach_ext_emit, behind
// reach_diff_scan of the chunk counts, writes the run-length records.  A class
// may be all of IPv4, so widths and their sums are 64-bit.  Plain C++
// throughout: vector stores, LDS and global atomics.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "k_reach_dev.hpp"
#include "kernels.hpp"

namespace cls {

namespace {

constexpr uint32_t kWaves = kReachBlock / 64u;

// Row i of the tile: its line after the tile's first, that line's (dir,
// probe) after the tile's first (q), its direction index, probe and endpoint,
// its class.  Two 32-bit divisions per lane; the lane's following rows
// advance by carries.
struct ExtRow {
    uint32_t line, q, d, p, s, k;
};
__device__ __forceinline__ ExtRow ext_row(const ReachExtTile& t, uint32_t i) {
    ExtRow r;
    r.line = i / t.K;
    r.k = i - r.line * t.K;
    const uint32_t x = t.s0 + r.line;            // < 2^18 + 2^30
    r.q = x / t.n_ep;
    r.s = x - r.q * t.n_ep;
    // (dir, probe) q steps behind (d0, p0): at most one direction further
    const uint32_t rem = t.n_probes - t.p0;      // >= 1
    r.d = r.q >= rem ? t.d0 + 1u : t.d0;
    r.p = r.q >= rem ? r.q - rem : t.p0 + r.q;
    return r;
}
__device__ __forceinline__ void ext_next(const ReachExtTile& t, ExtRow& r) {
    if (++r.k == t.K) {
        r.k = 0;
        ++r.line;
        if (++r.s == t.n_ep) {
            r.s = 0;
            ++r.q;
            if (++r.p == t.n_probes) {
                r.p = 0;
                ++r.d;
            }
        }
    }
}
// the direction (0 egress, 1 ingress) of direction index d
__device__ __forceinline__ uint32_t ext_dir(const ReachExtTile& t, uint32_t d) { return d ? t.dir_of[1] : t.dir_of[0]; }
// addresses of class k: up to 2^32
__device__ __forceinline__ unsigned long long ext_width(const ReachExtTile& t, uint32_t k) {
    return (k + 1u < t.K ? (unsigned long long)t.lo[k + 1u] : 1ull << 32) - t.lo[k];
}

// sum over the wave's 64 lanes of a 64-bit word
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor(uint32_t(v), o, 64), hi = __shfl_xor(uint32_t(v >> 32), o, 64);
        v += (unsigned long long)hi << 32 | lo;
    }
    return v;
}

// the remote address a: host-order u32, or the 16 network-order bytes of ::ffff:a
template <bool K16>
__device__ __forceinline__ auto ext_remote(uint32_t a) {
    if constexpr (K16) return uint4{0u, 0u, 0xFFFF0000u, __builtin_bswap32(a)};
    else return a;
}

// c ? a : b, word by word (a select of whole 16-B vectors goes through scratch)
__device__ __forceinline__ uint32_t ext_pick(bool c, uint32_t a, uint32_t b) { return c ? a : b; }
__device__ __forceinline__ uint4 ext_pick(bool c, const uint4& a, const uint4& b) {
    return uint4{c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z, c ? a.w : b.w};
}

template <bool K16>
__device__ __forceinline__ void ext_expand_body(const ReachExtTile& t, const ReachExtExpand& x) {
    using Addr = typename std::conditional<K16, uint4, uint32_t>::type;
    const Addr* ep = static_cast<const Addr*>(x.ep_addr);
    const uint32_t groups = (t.n + 3u) / 4u;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        ExtRow r = ext_row(t, 4u * g);
        // the line's endpoint, probe and direction, reloaded when a carry moves the line
        uint32_t pif = x.ep_if[r.s];
        Addr pa = ep[r.s];
        uint2 pb = x.probe[r.p];
        bool in = ext_dir(t, r.d) != 0u;
        uint32_t o_sif[4], o_dif[4], o_sp[4], o_dp[4], o_pr[4];
        Addr o_src[4], o_dst[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const Addr ra = ext_remote<K16>(t.lo[r.k]);
            o_sif[j] = in ? x.ext_if : pif;
            o_dif[j] = in ? pif : x.ext_if;
            o_src[j] = ext_pick(in, ra, pa);
            o_dst[j] = ext_pick(in, pa, ra);
            o_sp[j] = pb.x & 0xFFFFu;
            o_dp[j] = pb.x >> 16;
            o_pr[j] = pb.y & 0xFFu;
            // the next row -- only while rows remain (the tile's last row has
            // no successor to load: the rest of its group repeats it)
            if (j < 3 && 4u * g + j + 1u < t.n) {
                const uint32_t was = r.line;
                ext_next(t, r);
                if (r.line != was) {
                    pif = x.ep_if[r.s];
                    pa = ep[r.s];
                    pb = x.probe[r.p];
                    in = ext_dir(t, r.d) != 0u;
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
        reinterpret_cast<uint2*>(x.sport)[g] = uint2{o_sp[0] | o_sp[1] << 16, o_sp[2] | o_sp[3] << 16};
        reinterpret_cast<uint2*>(x.dport)[g] = uint2{o_dp[0] | o_dp[1] << 16, o_dp[2] | o_dp[3] << 16};
        reinterpret_cast<uint32_t*>(x.proto)[g] = o_pr[0] | o_pr[1] << 8 | o_pr[2] << 16 | o_pr[3] << 24;
    }
}
__global__ __launch_bounds__(256) void reach_ext_expand4(ReachExtTile t, ReachExtExpand x) {
    ext_expand_body<false>(t, x);
}
__global__ __launch_bounds__(256) void reach_ext_expand16(ReachExtTile t, ReachExtExpand x) {
    ext_expand_body<true>(t, x);
}

// The lane's four verdict bytes (one 4-B load; the tile's last, partial group
// byte by byte: nothing is read past the tile) and the byte of the row before
// them (unused at row 0, which starts a line).
struct ExtWords {
    uint32_t v4, live, prev;
};
__device__ __forceinline__ ExtWords ext_load(const ReachExtTile& t, const uint8_t* verdict, uint32_t i0) {
    ExtWords w{0u, 0u, 0u};
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

__global__ __launch_bounds__(kReachBlock) void reach_ext_count(ReachExtTile t, const uint8_t* verdict,
                                                               uint32_t* chunk_count, uint32_t* runs,
                                                               unsigned long long* allow, unsigned long long* hist) {
    __shared__ unsigned long long bins[4];                         // <= kReachChunk x 2^32 per chunk
    __shared__ uint32_t n_starts;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t chunks = (t.n + kReachChunk - 1u) / kReachChunk;
    for (uint32_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        if (threadIdx.x < 4u) bins[threadIdx.x] = 0ull;
        if (threadIdx.x == 4u) n_starts = 0u;
        __syncthreads();
        const uint32_t c0 = ch * kReachChunk;                      // the chunk's first row
        // the chunk in one (dir, probe): its histogram is binned in LDS (workgroup-uniform)
        const uint32_t q_c = ext_row(t, c0).q;
        const bool lds_bins = q_c == ext_row(t, min(c0 + kReachChunk - 1u, t.n - 1u)).q;
        const uint32_t i0 = c0 + 4u * threadIdx.x;                 // the lane's four rows
        const uint32_t w0 = i0 - 4u * lane;                        // the wave's 256
        if (w0 < t.n) {                                            // wave-uniform
            const ExtRow ra = ext_row(t, w0), rb = ext_row(t, min(w0 + 255u, t.n - 1u));
            const bool one_line = ra.line == rb.line, one_q = ra.q == rb.q;   // wave-uniform
            const ExtWords w = ext_load(t, verdict, i0);
            ExtRow r = ext_row(t, i0 < t.n ? i0 : w0);
            unsigned long long h[4] = {0ull, 0ull, 0ull, 0ull}, ok = 0ull;   // <= 4 x 2^32 each
            uint32_t starts = 0u, run = 0u, prev = w.prev;
            for (uint32_t j = 0; j < w.live; ++j) {
                const uint32_t v = byte_of(w.v4, j);
                const unsigned long long width = ext_width(t, r.k);
                const uint32_t st = (r.k == 0u || v != prev) ? 1u : 0u;
                prev = v;
                starts += st;
                run += st;
#pragma unroll
                for (uint32_t a = 0; a < 4u; ++a) h[a] += (v & 3u) == a ? width : 0ull;
                ok += v == 2u ? width : 0ull;                      // CLS_CONN_ALLOW
                // a wave across lines or (dir, probe)s: the lane's sums of one
                // of them, added when its rows leave it
                const uint32_t line = r.line, q = r.q;
                ext_next(t, r);
                const bool end = j + 1u == w.live;
                if (!one_line && (r.line != line || end)) {
                    if (runs && run) atomicAdd(&runs[line], run);
                    if (allow && ok) atomicAdd(&allow[line], ok);
                    run = 0u;
                    ok = 0ull;
                }
                if (!one_q && (r.q != q || end)) {
#pragma unroll
                    for (uint32_t a = 0; a < 4u; ++a) {
                        if (hist && h[a]) atomicAdd(&hist[4ull * q + a], h[a]);
                        h[a] = 0ull;
                    }
                }
            }
            if (chunk_count) {
                starts = wave_sum(starts);
                if (lane == 0u && starts) atomicAdd(&n_starts, starts);
            }
            if (one_line) {
                if (runs) {
                    run = wave_sum(run);
                    if (lane == 0u && run) atomicAdd(&runs[ra.line], run);
                }
                if (allow) {
                    ok = wave_sum64(ok);                           // <= 2^32
                    if (lane == 0u && ok) atomicAdd(&allow[ra.line], ok);
                }
            }
            if (hist && one_q) {
#pragma unroll
                for (uint32_t a = 0; a < 4u; ++a) h[a] = wave_sum64(h[a]);   // <= 256 x 2^32
                if (lane < 4u) {
                    const unsigned long long c = lane == 0u ? h[0] : lane == 1u ? h[1] : lane == 2u ? h[2] : h[3];
                    if (c) {
                        if (lds_bins) atomicAdd(&bins[lane], c);
                        else atomicAdd(&hist[4ull * ra.q + lane], c);
                    }
                }
            }
        }
        __syncthreads();
        if (hist && lds_bins && threadIdx.x < 4u && bins[threadIdx.x])
            atomicAdd(&hist[4ull * q_c + threadIdx.x], bins[threadIdx.x]);
        if (chunk_count && threadIdx.x == 4u) chunk_count[ch] = n_starts;
        __syncthreads();                                           // before the next chunk clears them
    }
}

__global__ __launch_bounds__(kReachBlock) void reach_ext_emit(ReachExtTile t, const uint8_t* verdict,
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
        const ExtWords w = ext_load(t, verdict, i0);
        ExtRow r = ext_row(t, i0 < t.n ? i0 : 0u);
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
        // inside the tile: the tile ends with a line)
        const uint32_t after = w.live && i0 + w.live < t.n ? uint32_t(verdict[i0 + w.live]) : 0u;
        for (uint32_t j = 0; j < w.live; ++j) {
            const uint32_t v = byte_of(w.v4, j);
            const bool start = (st >> j) & 1u;
            const uint32_t next = j + 1u < w.live ? byte_of(w.v4, j + 1u) : after;
            const bool last = r.k + 1u == t.K;
            const bool end = last || next != v;
            const uint32_t hi = last ? 0xFFFFFFFFu : t.lo[r.k + 1u] - 1u;
            if (start) {
                if (at < cap) {
                    const uint32_t w1 = (r.p & 0xFFFFu) | ext_dir(t, r.d) << 16 | v << 24;
                    const uint32_t lo = t.lo[r.k];
                    if (end) {
                        ranges[at] = uint4{r.s, w1, lo, hi};
                    } else {
                        // (addr_hi is the end row's: the two write disjoint words)
                        uint32_t* rec = reinterpret_cast<uint32_t*>(ranges + at);
                        *reinterpret_cast<uint2*>(rec) = uint2{r.s, w1};
                        rec[2] = lo;
                    }
                }
                ++at;
            }
            // at >= 1 here: the tile's first row is a start
            if (end && !start && at - 1ull < cap) reinterpret_cast<uint32_t*>(ranges + (at - 1ull))[3] = hi;
            ext_next(t, r);
        }
        __syncthreads();                                           // before the next chunk's wave counts
    }
}

}  // namespace

hipError_t launch_reach_ext_expand(const ReachExtTile& t, const ReachExtExpand& x, bool k16, int n_cu,
                                   hipStream_t s) {
    if (!t.n) return hipSuccess;
    const int grid = reach_grid((uint64_t(t.n) + 3) / 4, 256, n_cu);
    if (k16) hipLaunchKernelGGL(reach_ext_expand16, dim3(grid), dim3(256), 0, s, t, x);
    else hipLaunchKernelGGL(reach_ext_expand4, dim3(grid), dim3(256), 0, s, t, x);
    return hipGetLastError();
}

hipError_t launch_reach_ext_count(const ReachExtTile& t, const uint8_t* verdict, uint32_t* chunk_count,
                                  uint32_t* runs, unsigned long long* allow, unsigned long long* hist, int n_cu,
                                  hipStream_t s) {
    if (!t.n || (!chunk_count && !runs && !allow && !hist)) return hipSuccess;
    const int grid = reach_grid(t.n, kReachChunk, n_cu);
    hipLaunchKernelGGL(reach_ext_count, dim3(grid), dim3(kReachBlock), 0, s, t, verdict, chunk_count, runs, allow,
                       hist);
    return hipGetLastError();
}

hipError_t launch_reach_ext_emit(const ReachExtTile& t, const uint8_t* verdict, const unsigned long long* chunk_base,
                                 uint4* ranges, unsigned long long cap, int n_cu, hipStream_t s) {
    if (!t.n || !ranges || !cap) return hipSuccess;
    const int grid = reach_grid(t.n, kReachChunk, n_cu);
    hipLaunchKernelGGL(reach_ext_emit, dim3(grid), dim3(kReachBlock), 0, s, t, verdict, chunk_base, ranges, cap);
    return hipGetLastError();
}

}  // namespace cls
