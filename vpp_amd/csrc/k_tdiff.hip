// The table diff's kernels (kernels.hpp TDiffTile; tdiff.cpp cls_table_diff):
// a tile of whole rows of the joint class product, evaluated under table a
// (was, rule_a) and table b (now, rule_b).  tdiff_count histograms the (was,
// now) pairs, finds the tile's least differing cell, writes the two masked
// rule arrays cover_fold reduces per rule, and counts the run heads of every
// chunk; reach_diff_scan (k_reach_diff.hip) turns the chunk counts into each
// chunk's first record index; tdiff_emit writes the records there -- the order
// comes from the scan alone.  A run is a maximal stretch of differing cells of
// one row and one protocol with equal (was, now, rule_a, rule_b); the tile
// holds whole rows, so no run crosses it.  Tile-local indices are 32-bit.
// Plain C++ throughout: vector stores, LDS and global atomics.
#include <hip/hip_runtime.h>

#include "k_reach_dev.hpp"
#include "kernels.hpp"

namespace cls {

namespace {

constexpr uint32_t kWaves = kReachBlock / 64u;
constexpr uint32_t kNone = 0xFFFFFFFFu;

// Column j starts a protocol's stretch of a row / the column behind j's stretch.
__device__ __forceinline__ bool seg_start(const TDiffTile& q, uint32_t j) {
    return j == 0u || j == q.Kt || j >= q.Kt + q.Ku;
}
__device__ __forceinline__ uint32_t seg_end(const TDiffTile& q, uint32_t j) {
    return j < q.Kt ? q.Kt : j < q.Kt + q.Ku ? q.Kt + q.Ku : j + 1u;
}

// A cell's key: was | now << 8, and the two terminating rules.
struct Key {
    uint32_t vv, ra, rb;
};
__device__ __forceinline__ bool differs(uint32_t vv) { return (vv & 0xFFu) != (vv >> 8); }
__device__ __forceinline__ bool same_key(const Key& a, const Key& b) {
    return a.vv == b.vv && a.ra == b.ra && a.rb == b.rb;
}
__device__ __forceinline__ Key key_at(const TDiffCells& c, uint32_t i) {
    return Key{uint32_t(c.was[i]) | uint32_t(c.now[i]) << 8, c.rule_a[i], c.rule_b[i]};
}

// The lane's four cells from tile cell i0 (a multiple of 4) on: one 4-B load
// of each verdict array and one 16-B load of each rule array; the tile's last,
// partial group cell by cell (nothing is read past the tile).
struct Cells4 {
    Key k[4];
    uint32_t live;             // cells of the lane inside the tile
    uint32_t j0;               // the first one's column
    uint32_t diff, head;       // bit k: cell k differs / starts a run
};
__device__ __forceinline__ void cells_load(const TDiffTile& q, const TDiffCells& c, uint32_t i0, Cells4& r) {
    const uint32_t n = q.t.n;
    r.live = i0 >= n ? 0u : min(4u, n - i0);
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) r.k[k] = Key{0u, 0u, 0u};
    if (r.live == 4u) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(c.was + i0);
        const uint32_t v = *reinterpret_cast<const uint32_t*>(c.now + i0);
        const uint4 a = *reinterpret_cast<const uint4*>(c.rule_a + i0);
        const uint4 b = *reinterpret_cast<const uint4*>(c.rule_b + i0);
        r.k[0] = Key{(w & 0xFFu) | (v & 0xFFu) << 8, a.x, b.x};
        r.k[1] = Key{(w >> 8 & 0xFFu) | (v >> 8 & 0xFFu) << 8, a.y, b.y};
        r.k[2] = Key{(w >> 16 & 0xFFu) | (v >> 16 & 0xFFu) << 8, a.z, b.z};
        r.k[3] = Key{(w >> 24) | (v >> 24) << 8, a.w, b.w};
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
            if (k < r.live) r.k[k] = key_at(c, i0 + k);
    }
}

// diff and head of the lane's cells.  Every lane of the wave calls this (the
// cell before a lane's first is the lane below's last, through a shuffle; the
// wave's first lane reads it from memory).
__device__ __forceinline__ void cells_heads(const TDiffTile& q, const TDiffCells& c, uint32_t i0, uint32_t lane,
                                            Cells4& r) {
    Key p{uint32_t(__shfl_up(r.k[3].vv, 1, 64)), uint32_t(__shfl_up(r.k[3].ra, 1, 64)),
          uint32_t(__shfl_up(r.k[3].rb, 1, 64))};
    if (lane == 0u) p = r.live && i0 ? key_at(c, i0 - 1u) : Key{0u, 0u, 0u};
    r.j0 = i0 % q.t.T;
    r.diff = r.head = 0u;
    uint32_t j = r.j0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const bool d = k < r.live && differs(r.k[k].vv);
        const bool h = d && (seg_start(q, j) || !differs(p.vv) || !same_key(r.k[k], p));
        r.diff |= d ? 1u << k : 0u;
        r.head |= h ? 1u << k : 0u;
        p = r.k[k];
        j = j + 1u == q.t.T ? 0u : j + 1u;
    }
}

__global__ __launch_bounds__(kReachBlock) void tdiff_count(TDiffTile q, TDiffCells c, uint32_t none_a, uint32_t none_b,
                                                           uint32_t* mask_a, uint32_t* mask_b, uint32_t* chunk_count,
                                                           unsigned long long* pairs, unsigned long long* n_diff,
                                                           unsigned long long* first) {
    __shared__ uint32_t bins[16];
    __shared__ uint32_t n_heads, lo;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = q.t.n, chunks = (n + kReachChunk - 1u) / kReachChunk;
    if (threadIdx.x < 16u) bins[threadIdx.x] = 0u;
    if (threadIdx.x == 0u) {
        n_heads = 0u;
        lo = kNone;
    }
    __syncthreads();
    // a workgroup takes consecutive chunks: its bins and its least differing
    // cell reach global memory once
    const uint32_t per = (chunks + gridDim.x - 1u) / gridDim.x;
    const uint32_t ch_a = min(blockIdx.x * per, chunks), ch_b = min(ch_a + per, chunks);
    for (uint32_t ch = ch_a; ch < ch_b; ++ch) {
        const uint32_t i0 = ch * kReachChunk + 4u * threadIdx.x;   // the lane's four cells
        const uint32_t w0 = i0 - 4u * lane;                        // the wave's 256
        if (w0 < n) {                                              // wave-uniform
            Cells4 r;
            cells_load(q, c, i0, r);
            cells_heads(q, c, i0, lane, r);
            // the masked rules: the rule where the cell differs, the sentinel where not
            uint32_t ma[4], mb[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                ma[k] = r.diff >> k & 1u ? r.k[k].ra : none_a;
                mb[k] = r.diff >> k & 1u ? r.k[k].rb : none_b;
            }
            if (r.live == 4u) {
                *reinterpret_cast<uint4*>(mask_a + i0) = uint4{ma[0], ma[1], ma[2], ma[3]};
                *reinterpret_cast<uint4*>(mask_b + i0) = uint4{mb[0], mb[1], mb[2], mb[3]};
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k)
                    if (k < r.live) {
                        mask_a[i0 + k] = ma[k];
                        mask_b[i0 + k] = mb[k];
                    }
            }
            // run heads and the least differing cell, once per wave
            uint32_t wh = 0u;
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) wh += __popcll(__ballot(r.head >> k & 1u));
            if (chunk_count && lane == 0u && wh) atomicAdd(&n_heads, wh);
            const unsigned long long dl = __ballot(r.diff != 0u);
            if (dl && lane == uint32_t(__ffsll((long long)dl)) - 1u)
                atomicMin(&lo, i0 + uint32_t(__ffs(int(r.diff))) - 1u);
            // the (was, now) bins: a wave of one pair adds once, any other one add per pair it holds
            uint32_t code[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) code[k] = 4u * (r.k[k].vv & 3u) + (r.k[k].vv >> 8 & 3u);
            const uint32_t cf = __builtin_amdgcn_readfirstlane(code[0]);   // lane 0 holds a cell
            bool same = true;
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) same = same && (k >= r.live || code[k] == cf);
            if (__all(same)) {
                if (lane == 0u) atomicAdd(&bins[cf], min(256u, n - w0));
            } else {
                uint32_t mine = 0u;
                for (uint32_t f = 0; f < 16u; ++f) {
                    uint32_t cnt = 0u;
#pragma unroll
                    for (uint32_t k = 0; k < 4u; ++k) cnt += __popcll(__ballot(k < r.live && code[k] == f));
                    if (lane == f) mine = cnt;
                }
                if (lane < 16u && mine) atomicAdd(&bins[lane], mine);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0u) {
            if (chunk_count) chunk_count[ch] = n_heads;
            n_heads = 0u;
        }
        __syncthreads();                                           // before the next chunk's adds
    }
    if (threadIdx.x < 16u) {
        const uint32_t b = bins[threadIdx.x];
        if (pairs && b) atomicAdd(&pairs[threadIdx.x], (unsigned long long)b);
    }
    if (threadIdx.x == 0u) {
        unsigned long long d = 0ull;
        for (uint32_t f = 0; f < 16u; ++f) d += (f >> 2) != (f & 3u) ? bins[f] : 0u;
        if (n_diff && d) atomicAdd(n_diff, d);
        if (lo != kNone) atomicMin(first, q.t.c0 + lo);
    }
}

// The record of the run of `len` cells from tile cell i on, key k, as two 16-B
// stores: {src_lo, src_hi, dst_lo, dst_hi}, {port_lo | port_hi << 16, proto |
// was << 8 | now << 16, rule_a, rule_b}.
__device__ __forceinline__ void rec_store(const TDiffTile& q, uint32_t i, uint32_t len, const Key& k, uint4* rec) {
    const uint32_t row = i / q.t.T, j = i - row * q.t.T, jt = j + len - 1u;      // the tail's column
    const unsigned long long sd = q.t.c0 / q.t.T + row;                           // the tile starts a row
    const unsigned long long s64 = sd / q.t.Kd;
    const uint32_t s = uint32_t(s64), d = uint32_t(sd - s64 * q.t.Kd);
    const uint32_t col = q.t.col[j];
    const uint32_t port_hi = jt + 1u == seg_end(q, j) ? 0xFFFFu : (q.t.col[jt + 1u] & 0xFFFFu) - 1u;
    rec[0] = uint4{q.t.slo[s], s + 1u < q.Ks ? q.t.slo[s + 1u] - 1u : 0xFFFFFFFFu, q.t.dlo[d],
                   d + 1u < q.t.Kd ? q.t.dlo[d + 1u] - 1u : 0xFFFFFFFFu};
    rec[1] = uint4{(col & 0xFFFFu) | port_hi << 16, (col >> 16 & 0xFFu) | (k.vv & 0xFFFFu) << 8, k.ra, k.rb};
}

__global__ __launch_bounds__(kReachBlock) void tdiff_emit(TDiffTile q, TDiffCells c, const uint32_t* chunk_count,
                                                          const unsigned long long* chunk_base, uint4* rec,
                                                          unsigned long long cap) {
    __shared__ uint32_t wave_n[kWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n = q.t.n, chunks = (n + kReachChunk - 1u) / kReachChunk;
    for (uint32_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        // workgroup-uniform: a chunk without a head, or whose records all lie past cap, writes nothing
        if (!chunk_count[ch]) continue;
        const unsigned long long first = chunk_base[ch];
        if (first >= cap) continue;
        const uint32_t i0 = ch * kReachChunk + 4u * threadIdx.x;   // the lane's four cells
        const uint32_t w0 = i0 - 4u * lane;                        // the wave's 256
        Cells4 r;
        r.live = r.diff = r.head = r.j0 = 0u;
        uint32_t below = 0u, mine = 0u;
        if (w0 < n) {                                              // wave-uniform
            cells_load(q, c, i0, r);
            cells_heads(q, c, i0, lane, r);
            // the heads before the lane's in its wave (cell order: the lower lanes' cells come first), and the wave's
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                const unsigned long long m = __ballot(r.head >> k & 1u);
                below += __popcll(m & ((1ull << lane) - 1ull));
                mine += __popcll(m);
            }
        }
        if (lane == 0u) wave_n[wave] = mine;
        __syncthreads();
        unsigned long long at = first + below;
        for (uint32_t k = 0; k < wave; ++k) at += wave_n[k];
        if (mine) {                                                // wave-uniform
            // a run ends in front of the next break: a head, a cell that does
            // not differ, or the end of the tile (which ends a row)
            const uint32_t brk = (r.head | ~r.diff) & 0xFu;        // cells past the tile: diff 0
            const unsigned long long lanes = __ballot(brk != 0u);
            const unsigned long long later = lane == 63u ? 0ull : lanes & ~((2ull << lane) - 1ull);
            const uint32_t nl = later ? uint32_t(__ffsll((long long)later)) - 1u : 0u;
            const uint32_t nk = __shfl(brk ? uint32_t(__ffs(int(brk))) - 1u : 0u, int(nl), 64);
            const uint32_t after = later ? w0 + 4u * nl + nk : kNone;             // the first break behind this lane
            // the wave's last head may run on behind the wave: at most one run, which the wave follows together
            const uint32_t top = r.head ? 31u - uint32_t(__clz(int(r.head))) : 0u;
            const bool open = r.head && !(brk >> (top + 1u)) && after == kNone;
            const unsigned long long ol = __ballot(open);
            uint32_t open_end = 0u;
            if (ol) {                                              // wave-uniform
                const int src = __ffsll((long long)ol) - 1;
                const uint32_t hk = uint32_t(__shfl(int(top), src, 64));
                const uint32_t hi = uint32_t(__shfl(int(i0), src, 64)) + hk;
                Key kk = r.k[0];
#pragma unroll
                for (uint32_t k = 1; k < 4u; ++k)
                    if (top == k) kk = r.k[k];
                kk = Key{uint32_t(__shfl(int(kk.vv), src, 64)), uint32_t(__shfl(int(kk.ra), src, 64)),
                         uint32_t(__shfl(int(kk.rb), src, 64))};
                const uint32_t hj = hi % q.t.T;
                const uint32_t limit = hi + (seg_end(q, hj) - hj);            // <= n: the tile holds whole rows
                open_end = limit;
                for (uint32_t p = w0 + 256u; p < limit; p += 256u) {
                    Cells4 x;
                    cells_load(q, c, p + 4u * lane, x);
                    uint32_t bad = 0u;
#pragma unroll
                    for (uint32_t k = 0; k < 4u; ++k)
                        bad |= p + 4u * lane + k < limit && !same_key(x.k[k], kk) ? 1u << k : 0u;
                    const unsigned long long bl = __ballot(bad != 0u);
                    if (bl) {
                        const int fl = __ffsll((long long)bl) - 1;
                        open_end = p + 4u * uint32_t(fl) + uint32_t(__shfl(__ffs(int(bad)) - 1, fl, 64));
                        break;
                    }
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                if (!(r.head >> k & 1u)) continue;
                const uint32_t rest = brk >> (k + 1u);             // breaks behind k in this lane
                const uint32_t stop = rest ? i0 + k + uint32_t(__ffs(int(rest))) : after != kNone ? after : open_end;
                if (at < cap) rec_store(q, i0 + k, stop - (i0 + k), r.k[k], rec + 2ull * at);
                ++at;
            }
        }
        __syncthreads();                                           // before the next chunk's wave counts
    }
}

}  // namespace

hipError_t launch_tdiff_count(const TDiffTile& q, const TDiffCells& c, uint32_t none_a, uint32_t none_b,
                              uint32_t* mask_a, uint32_t* mask_b, uint32_t* chunk_count, unsigned long long* pairs,
                              unsigned long long* n_diff, unsigned long long* first, int n_cu, hipStream_t s) {
    if (!q.t.n) return hipSuccess;
    // two workgroups of kReachBlock fill a CU: no more, so that each has a long run of chunks
    const int grid = std::min(reach_grid(q.t.n, kReachChunk, n_cu), 2 * std::max(1, n_cu));
    hipLaunchKernelGGL(tdiff_count, dim3(grid), dim3(kReachBlock), 0, s, q, c, none_a, none_b, mask_a, mask_b,
                       chunk_count, pairs, n_diff, first);
    return hipGetLastError();
}

hipError_t launch_tdiff_emit(const TDiffTile& q, const TDiffCells& c, const uint32_t* chunk_count,
                             const unsigned long long* chunk_base, uint4* rec, unsigned long long cap, int n_cu,
                             hipStream_t s) {
    if (!q.t.n || !rec || !cap) return hipSuccess;
    const int grid = reach_grid(q.t.n, kReachChunk, n_cu);
    hipLaunchKernelGGL(tdiff_emit, dim3(grid), dim3(kReachBlock), 0, s, q, c, chunk_count, chunk_base, rec, cap);
    return hipGetLastError();
}

}  // namespace cls
