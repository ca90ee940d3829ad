// The hop closure's kernels (kernels.hpp; reach.cpp cls_reach_hops):
// reach_adj_fold turns a tile's verdict bytes into bits of the adjacency
// bitmap, reach_hops_bfs runs the level-synchronous breadth-first search from
// every source over it, bit-parallel, and writes every output.  Plain C++
// throughout: ballots, vector stores, LDS and global atomics.  No workgroup
// waits for another, and every loop has a bound of its own.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "k_reach_dev.hpp"
#include "kernels.hpp"

namespace cls {

namespace {

using u64 = unsigned long long;

// A wave takes 64 consecutive cells of the tile, one per lane.  Lanes with
// the same word (source s, d >> 6) are a run of consecutive lanes -- the rest
// of a row, or its start -- unless N^2 < 64 and a later probe comes back to
// the word.  Per touched word: the run's ALLOW ballot, shifted to the run's
// first destination bit (a word whose lanes are no single run: an OR over the
// wave), and one atomic OR -- different probes, and the waves on either side
// of a row end, meet in the same word.
__global__ __launch_bounds__(256) void reach_adj_fold(ReachTile t, const uint8_t* verdict, u64* adj, uint32_t W) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves = gridDim.x * (blockDim.x / 64u);
    const uint32_t chunks = (t.n + 63u) / 64u;
    for (uint32_t ch = blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; ch < chunks; ch += waves) {
        const uint32_t i = ch * 64u + lane;                        // < 2^30 + 64
        const bool in = i < t.n;
        bool allow = false;
        uint32_t key = 0u, d = 0u;
        if (in) {
            const ReachCell c = reach_cell(t, i);
            const ReachRow r = reach_row(t, c.row);
            d = c.d;
            key = r.s * W + (d >> 6);                              // < N W <= 2^24
            allow = verdict[i] == 2u && r.s != d;                  // CLS_CONN_ALLOW, off the diagonal
        }
        u64 todo = __ballot(allow);
        while (todo) {                                             // one turn per touched word: at most 64
            const int l0 = __ffsll(todo) - 1;                      // the word's first ALLOW lane
            const uint32_t k = __shfl(key, l0);
            const u64 all = __ballot(in && key == k);
            const u64 m = __ballot(allow && key == k);
            const u64 run = all >> (__ffsll(all) - 1);
            u64 word;
            if ((run & (run + 1ull)) == 0ull)                      // one run: lane l holds bit (d(l0) & 63) + l - l0
                word = (m >> l0) << (__shfl(d, l0) & 63u);
            else
                word = wave_or64(allow && key == k ? 1ull << (d & 63u) : 0ull);
            if (lane == uint32_t(l0)) atomicOr(&adj[k], word);
            todo &= ~m;
        }
    }
}

// A workgroup owns R consecutive source rows from level 1 to the end.  LDS:
// reached, front (the last level's new bits), next (this level's), R rows of
// W words each; uni, the union of the R frontiers; lvl, the workgroup's
// pairs per hops value.  A level: for every j in uni the row adj[j] is loaded
// once -- thread = word w of a chunk of CW = 2^cw_log2 columns, the 256 / CW
// thread groups taking j's bits in turn -- and ORed into the accumulators of
// the rows that have j in their frontier; next = acc & ~reached.  The loop
// ends after H levels or when the workgroup's frontier is empty.
template <int R>
__global__ __launch_bounds__(kHopsBlock) void reach_hops_bfs(uint32_t N, uint32_t W, uint32_t H, uint32_t cw_log2,
                                                             const u64* adj, uint8_t* hops, uint32_t* reach,
                                                             uint32_t* exposed, u64* levels, u64* closure) {
    extern __shared__ u64 hops_lds[];
    const uint32_t RW = uint32_t(R) * W;
    u64* reached = hops_lds;
    u64* front = reached + RW;
    u64* next = front + RW;
    u64* uni = next + RW;
    uint32_t* lvl = reinterpret_cast<uint32_t*>(uni + W);          // [256]
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    const uint32_t s0 = blockIdx.x * uint32_t(R);                  // the first source row; s0 < N
    const uint32_t rows = min(uint32_t(R), N - s0);
    for (uint32_t i = t; i < RW; i += kHopsBlock) {
        reached[i] = 0ull;
        front[i] = 0ull;
        next[i] = 0ull;
    }
    lvl[t] = 0u;
    __syncthreads();
    if (t < rows) {
        const uint32_t s = s0 + t;
        reached[t * W + (s >> 6)] = front[t * W + (s >> 6)] = 1ull << (s & 63u);
        if (hops) hops[size_t(s) * N + s] = 0;
    }
    __syncthreads();
    const uint32_t CW = 1u << cw_log2, G = kHopsBlock >> cw_log2, lw = t & (CW - 1u), jg = t >> cw_log2;
    for (uint32_t L = 1; L <= H; ++L) {
        u64 any = 0ull;
        for (uint32_t w = t; w < W; w += kHopsBlock) {
            u64 u = 0ull;
#pragma unroll
            for (int r = 0; r < R; ++r) u |= front[r * W + w];
            uni[w] = u;
            any |= u;
        }
        if (!__syncthreads_or(any != 0ull)) break;                 // (uniform) nothing left to expand
        for (uint32_t c0 = 0; c0 < W; c0 += CW) {
            const uint32_t w = c0 + lw;
            const bool valid = w < W;
            u64 acc[R];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = 0ull;
            for (uint32_t jw = 0; jw < W; ++jw) {
                const u64 u = uni[jw];
                if (!u) continue;                                  // (uniform)
                u64 fr[R];
#pragma unroll
                for (int r = 0; r < R; ++r) fr[r] = front[r * W + jw];
                // four of the group's bits at a time: their loads are in flight
                // together (j = 64 jw + b < N: a frontier holds destinations only)
                for (uint32_t b0 = jg; b0 < 64u; b0 += 4u * G) {
                    bool on[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t b = b0 + uint32_t(k) * G;
                        on[k] = b < 64u && ((u >> (b & 63u)) & 1ull);
                    }
                    if (!(on[0] || on[1] || on[2] || on[3])) continue;     // (a sparse frontier: mostly)
                    u64 a[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        a[k] = valid && on[k] ? adj[size_t(64u * jw + b0 + uint32_t(k) * G) * W + w] : 0ull;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (!on[k]) continue;
                        const uint32_t b = b0 + uint32_t(k) * G;           // < 64
#pragma unroll
                        for (int r = 0; r < R; ++r)
                            if ((fr[r] >> b) & 1ull) acc[r] |= a[k];
                    }
                }
            }
            if (valid) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const u64 v = acc[r] & ~reached[r * W + w];
                    if (v) atomicOr(&next[r * W + w], v);
                }
            }
        }
        __syncthreads();
        uint32_t cnt = 0u;
        for (uint32_t i = t; i < RW; i += kHopsBlock) {
            const u64 nx = next[i];
            next[i] = 0ull;
            front[i] = nx;
            reached[i] |= nx;
            cnt += uint32_t(__popcll(nx));
        }
        cnt = wave_sum(cnt);
        if (lane == 0u && cnt) atomicAdd(&lvl[L], cnt);
        __syncthreads();
        // the level's hops bytes: a wave per word, a lane per destination
        if (hops) {
            for (uint32_t i = wv; i < RW; i += kHopsBlock / 64u) {
                const u64 word = front[i];
                if (!word) continue;                               // (uniform)
                const uint32_t r = i / W, w = i - r * W;
                if ((word >> lane) & 1ull) hops[size_t(s0 + r) * N + 64u * w + lane] = uint8_t(L);
            }
        }
    }
    // the rows' other outputs, all of them functions of `reached`
    if (closure)
        for (uint32_t i = t; i < rows * W; i += kHopsBlock) closure[size_t(s0) * W + i] = reached[i];
    if (hops) {
        for (uint32_t i = wv; i < rows * W; i += kHopsBlock / 64u) {
            const uint32_t r = i / W, w = i - r * W, d = 64u * w + lane;
            if (d < N && !((reached[i] >> lane) & 1ull)) hops[size_t(s0 + r) * N + d] = 255;   // CLS_HOPS_NONE
        }
    }
    for (uint32_t r = wv; r < rows; r += kHopsBlock / 64u) {
        uint32_t c = 0u;
        for (uint32_t w = lane; w < W; w += 64u) c += uint32_t(__popcll(reached[r * W + w]));
        c = wave_sum(c);                                           // the row's destinations and itself
        if (lane == 0u) {
            if (reach) reach[s0 + r] = c - 1u;
            atomicAdd(&lvl[0], 1u);
            if (N - c) atomicAdd(&lvl[255], N - c);
        }
    }
    if (exposed) {
        for (uint32_t d = t; d < N; d += kHopsBlock) {
            uint32_t c = 0u;
            for (uint32_t r = 0; r < rows; ++r) c += uint32_t((reached[r * W + (d >> 6)] >> (d & 63u)) & 1ull);
            if (d - s0 < rows) --c;                                // d is one of the rows: its own bit
            if (c) atomicAdd(&exposed[d], c);
        }
    }
    __syncthreads();
    if (levels && lvl[t]) atomicAdd(&levels[t], u64(lvl[t]));
}

}  // namespace

hipError_t launch_reach_adj_fold(const ReachTile& t, const uint8_t* verdict, unsigned long long* adj, int n_cu,
                                 hipStream_t s) {
    if (!t.n) return hipSuccess;
    const int grid = reach_grid(t.n, 256, n_cu);
    hipLaunchKernelGGL(reach_adj_fold, dim3(grid), dim3(256), 0, s, t, verdict, adj, (t.n_ep + 63u) / 64u);
    return hipGetLastError();
}

size_t reach_hops_lds(uint32_t n_ep, uint32_t rows) {
    const size_t W = (size_t(n_ep) + 63) / 64;
    return (3 * size_t(rows) * W + W) * 8 + 256 * 4;
}

uint32_t reach_hops_rows(uint32_t n_ep, uint32_t want) {
    uint32_t rows = want == 8 || want == 16 ? want : 4;
    while (rows > 4 && reach_hops_lds(n_ep, rows) > 65536) rows /= 2;
    return rows;
}

hipError_t launch_reach_hops_bfs(uint32_t n_ep, uint32_t max_hops, uint32_t rows, const unsigned long long* adj,
                                 uint8_t* hops, uint32_t* reach, uint32_t* exposed, unsigned long long* levels,
                                 unsigned long long* closure, hipStream_t s) {
    if (!n_ep) return hipSuccess;
    const uint32_t W = (n_ep + 63u) / 64u;
    uint32_t cw_log2 = 0;
    while ((1u << cw_log2) < W && (1u << cw_log2) < kHopsBlock) ++cw_log2;
    const size_t lds = reach_hops_lds(n_ep, rows);
    if (lds > 65536 || max_hops < 1 || max_hops > 254) return hipErrorInvalidValue;
    const dim3 grid((n_ep + rows - 1) / rows), block(kHopsBlock);
    if (rows == 4)
        hipLaunchKernelGGL(reach_hops_bfs<4>, grid, block, lds, s, n_ep, W, max_hops, cw_log2, adj, hops, reach, exposed,
                           levels, closure);
    else if (rows == 8)
        hipLaunchKernelGGL(reach_hops_bfs<8>, grid, block, lds, s, n_ep, W, max_hops, cw_log2, adj, hops, reach, exposed,
                           levels, closure);
    else if (rows == 16)
        hipLaunchKernelGGL(reach_hops_bfs<16>, grid, block, lds, s, n_ep, W, max_hops, cw_log2, adj, hops, reach,
                           exposed, levels, closure);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace cls
