// The rule coverage sweep's kernels (kernels.hpp CoverTile; cover.cpp
// cls_table_cover).  cover_expand4 / cover_expand16 write a tile's cells --
// (source class, destination class, column) in cell order, each one's lowest
// packet -- as the arrays of a device classify batch; cover_fold reduces the
// tile's terminating rules to the least global cell index and the cell count
// per rule; cover_finish, once per call, turns each rule's least cell into its
// witness record.  Cell indices are 64-bit (up to 2^40) until reduced to the
// offset in the tile.  Plain C++ throughout: vector stores, LDS and global
// atomics.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "k_reach_dev.hpp"
#include "kernels.hpp"

namespace cls {

namespace {

constexpr unsigned long long kNoCell = ~0ull;

// Cell c: its source class, destination class and column.  Two 64-bit
// divisions per lane; the lane's following cells advance by carries.
struct CoverCell {
    uint32_t s, d, j;
};
__device__ __forceinline__ CoverCell cover_cell(const CoverTile& t, unsigned long long c) {
    CoverCell r;
    const unsigned long long sd = c / t.T;                       // < 2^40
    r.j = uint32_t(c - sd * t.T);
    const unsigned long long s = sd / t.Kd;
    r.s = uint32_t(s);
    r.d = uint32_t(sd - s * t.Kd);
    return r;
}
__device__ __forceinline__ void cover_next(const CoverTile& t, CoverCell& r) {
    if (++r.j == t.T) {
        r.j = 0;
        if (++r.d == t.Kd) {
            r.d = 0;
            ++r.s;
        }
    }
}

// the address a: host-order u32, or the 16 network-order bytes of ::ffff:a
template <bool K16>
__device__ __forceinline__ auto cover_addr(uint32_t a) {
    if constexpr (K16) return uint4{0u, 0u, 0xFFFF0000u, __builtin_bswap32(a)};
    else return a;
}

// Four cells per lane in reach_expand's store shape; the tile's last group is
// padded by repeating its last cell (the arrays hold whole groups).
template <bool K16>
__device__ __forceinline__ void cover_expand_body(const CoverTile& t, void* src, void* dst, uint16_t* dport,
                                                  uint8_t* proto) {
    using Addr = typename std::conditional<K16, uint4, uint32_t>::type;
    const uint32_t groups = (t.n + 3u) / 4u;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        CoverCell r = cover_cell(t, t.c0 + 4u * g);
        uint32_t sa = t.slo[r.s], da = t.dlo[r.d];
        Addr o_src[4], o_dst[4];
        uint32_t o_col[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o_src[k] = cover_addr<K16>(sa);
            o_dst[k] = cover_addr<K16>(da);
            o_col[k] = t.col[r.j];
            // the next cell, only while cells remain in the tile
            if (k < 3 && 4u * g + k + 1u < t.n) {
                cover_next(t, r);
                if (r.j == 0u) {
                    sa = t.slo[r.s];
                    da = t.dlo[r.d];
                }
            }
        }
        if constexpr (K16) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                static_cast<uint4*>(src)[4u * g + k] = o_src[k];
                static_cast<uint4*>(dst)[4u * g + k] = o_dst[k];
            }
        } else {
            static_cast<uint4*>(src)[g] = uint4{o_src[0], o_src[1], o_src[2], o_src[3]};
            static_cast<uint4*>(dst)[g] = uint4{o_dst[0], o_dst[1], o_dst[2], o_dst[3]};
        }
        reinterpret_cast<uint2*>(dport)[g] = uint2{(o_col[0] & 0xFFFFu) | o_col[1] << 16,
                                                   (o_col[2] & 0xFFFFu) | o_col[3] << 16};
        reinterpret_cast<uint32_t*>(proto)[g] = (o_col[0] >> 16 & 0xFFu) | (o_col[1] >> 16 & 0xFFu) << 8 |
                                                (o_col[2] >> 16 & 0xFFu) << 16 | (o_col[3] >> 16 & 0xFFu) << 24;
    }
}
__global__ __launch_bounds__(256) void cover_expand4(CoverTile t, void* src, void* dst, uint16_t* dport,
                                                     uint8_t* proto) {
    cover_expand_body<false>(t, src, dst, dport, proto);
}
__global__ __launch_bounds__(256) void cover_expand16(CoverTile t, void* src, void* dst, uint16_t* dport,
                                                      uint8_t* proto) {
    cover_expand_body<true>(t, src, dst, dport, proto);
}

// One run of equal rules: `len` cells from global cell `first` on terminate at
// rule r.  The least cell only ever falls, so a plain read that is already at
// or below `first` makes the atomic unnecessary (a stale read is above the
// true value, never below it): after a rule's first tile its minimum costs a
// load.  r < n_out holds for every rule index the classify kernels write; the
// test keeps a wrong one inside the arrays.
// kBins: the counts go to the workgroup's LDS bins (u32: a workgroup's span is
// below 2^32 cells) instead of global memory.
template <bool kBins>
__device__ __forceinline__ void cover_emit(uint32_t r, unsigned long long first, unsigned long long len,
                                           uint32_t n_out, unsigned long long* minc, unsigned long long* cnt,
                                           uint32_t* bins) {
    if (r >= n_out || !len) return;
    if (first < minc[r]) atomicMin(&minc[r], first);
    if constexpr (kBins) atomicAdd(&bins[r], uint32_t(len));
    else atomicAdd(&cnt[r], len);
}

constexpr uint32_t kFoldWaves = kReachBlock / 64u;
constexpr uint32_t kCoverBins = 15360u;      // u32 count bins per workgroup: 60 KiB of LDS, two workgroups per CU

// A workgroup takes a contiguous span of the tile, each of its waves a
// contiguous part of that in steps of 256 cells (four per lane, one 16-B
// load).  A wave carries the run it is in -- rule, first cell, length -- across
// its steps in wave-uniform registers: a step whose cells all equal the carried
// rule adds 256 to the length and touches no memory.  A step with more than one
// rule closes the carried run and emits each of its own runs from the run's
// head lane (the run's length from the next head's position, found with a
// ballot and one shuffle).  At the end the waves' open runs meet in LDS and one
// lane merges neighbours of equal rule before emitting: a rule that owns the
// workgroup's whole span costs one atomic add per workgroup and tile.
// kBins (R + 1 <= kCoverBins): every count goes to n_out u32 bins in LDS first
// and each non-zero bin is added to global memory once per workgroup -- where
// the columns alternate between a few rules the runs are short, and one global
// atomic per run is the per-cell atomic the wave reduction was meant to avoid.
template <bool kBins>
__device__ __forceinline__ void cover_fold_body(unsigned long long c0, uint32_t n, const uint32_t* rule,
                                                uint32_t n_out, unsigned long long* minc, unsigned long long* cnt) {
    extern __shared__ uint32_t bins[];
    __shared__ uint32_t w_rule[kFoldWaves], w_len[kFoldWaves], w_first[kFoldWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if constexpr (kBins) {
        for (uint32_t i = threadIdx.x; i < n_out; i += blockDim.x) bins[i] = 0u;
        __syncthreads();
    }
    // cells per wave: whole steps, so that every step's loads are 16-B aligned
    const uint32_t waves = gridDim.x * kFoldWaves;
    const uint32_t span = uint32_t(((uint64_t(n) + waves - 1u) / waves + 255u) & ~uint64_t(255));
    const uint64_t b64 = uint64_t(blockIdx.x * kFoldWaves + wave) * span;
    const uint32_t begin = uint32_t(b64 < n ? b64 : n), end = uint32_t(b64 + span < n ? b64 + span : n);
    uint32_t cr = 0xFFFFFFFFu, cfirst = 0u, clen = 0u;          // the open run (clen 0: none)
    for (uint32_t i0 = begin; i0 < end; i0 += 256u) {
        const uint32_t step = min(256u, end - i0);
        const uint32_t p0 = 4u * lane;
        const uint32_t live = p0 >= step ? 0u : min(4u, step - p0);
        uint32_t r[4] = {0u, 0u, 0u, 0u};
        if (live == 4u) {
            const uint4 v = *reinterpret_cast<const uint4*>(rule + i0 + p0);
            r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
        } else {
            for (uint32_t k = 0; k < live; ++k) r[k] = rule[i0 + p0 + k];
        }
        const uint32_t rf = __builtin_amdgcn_readfirstlane(r[0]);     // lane 0 always holds a cell
        bool same = true;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) same = same && (k >= live || r[k] == rf);
        if (__all(same)) {                                            // wave-uniform
            if (clen && rf == cr) {
                clen += step;
            } else {
                if (lane == 0u) cover_emit<kBins>(cr, c0 + cfirst, clen, n_out, minc, cnt, bins);
                cr = rf; cfirst = i0; clen = step;
            }
            continue;
        }
        if (lane == 0u) cover_emit<kBins>(cr, c0 + cfirst, clen, n_out, minc, cnt, bins);
        clen = 0u;
        // heads: cells whose rule differs from the cell before (the step's first cell is one)
        const uint32_t before = __shfl_up(r[3], 1, 64);
        uint32_t hm = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const bool h = k < live && (k == 0u ? (lane == 0u || r[0] != before) : r[k] != r[k - 1u]);
            hm |= h ? 1u << k : 0u;
        }
        const unsigned long long lanes = __ballot(hm != 0u);
        const unsigned long long later = lane == 63u ? 0ull : lanes & ~((2ull << lane) - 1ull);
        const uint32_t nl = later ? uint32_t(__ffsll((long long)later)) - 1u : 0u;
        const uint32_t nk = __shfl(hm ? uint32_t(__ffs(int(hm))) - 1u : 0u, int(nl), 64);
        const uint32_t after = later ? 4u * nl + nk : step;           // the first head behind this lane
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            if (!(hm >> k & 1u)) continue;
            const uint32_t rest = hm >> (k + 1u);                     // heads behind k in this lane
            const uint32_t stop = rest ? p0 + k + uint32_t(__ffs(int(rest))) : after;
            cover_emit<kBins>(r[k], c0 + i0 + p0 + k, stop - (p0 + k), n_out, minc, cnt, bins);
        }
    }
    if (lane == 0u) {
        w_rule[wave] = cr; w_len[wave] = clen; w_first[wave] = cfirst;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        // the waves' spans are adjacent and ascending: merge neighbours of equal rule
        uint32_t mr = 0u, mf = 0u;
        unsigned long long ml = 0ull;
        for (uint32_t w = 0; w < kFoldWaves; ++w) {
            if (!w_len[w]) continue;
            if (ml && w_rule[w] == mr && mf + ml == w_first[w]) {
                ml += w_len[w];
            } else {
                cover_emit<kBins>(mr, c0 + mf, ml, n_out, minc, cnt, bins);
                mr = w_rule[w]; mf = w_first[w]; ml = w_len[w];
            }
        }
        cover_emit<kBins>(mr, c0 + mf, ml, n_out, minc, cnt, bins);
    }
    if constexpr (kBins) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_out; i += blockDim.x)
            if (const uint32_t b = bins[i]) atomicAdd(&cnt[i], (unsigned long long)b);
    }
}
__global__ __launch_bounds__(kReachBlock) void cover_fold(unsigned long long c0, uint32_t n, const uint32_t* rule,
                                                          uint32_t n_out, unsigned long long* minc,
                                                          unsigned long long* cnt) {
    cover_fold_body<false>(c0, n, rule, n_out, minc, cnt);
}
__global__ __launch_bounds__(kReachBlock) void cover_fold_bins(unsigned long long c0, uint32_t n, const uint32_t* rule,
                                                               uint32_t n_out, unsigned long long* minc,
                                                               unsigned long long* cnt) {
    cover_fold_body<true>(c0, n, rule, n_out, minc, cnt);
}

// Rule k's least cell -> its witness {src, dst, dport | proto << 16 | live <<
// 24, 0}, its live byte, and the dead rules below R counted once per wave.
__global__ __launch_bounds__(256) void cover_finish(CoverTile t, const unsigned long long* minc, uint32_t n_out,
                                                    uint8_t* live_out, uint4* witness, uint32_t* n_dead) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long m = k < n_out ? minc[k] : 0ull;
    const bool live = m != kNoCell;
    if (k < n_out) {
        uint4 w{0u, 0u, 0u, 0u};
        if (live) {
            const CoverCell c = cover_cell(t, m);
            w = uint4{t.slo[c.s], t.dlo[c.d], (t.col[c.j] & 0xFFFFFFu) | 1u << 24, 0u};
        }
        if (witness) witness[k] = w;
        if (live_out) live_out[k] = live ? 1u : 0u;
    }
    const unsigned long long dead = __ballot(k + 1u < n_out && !live);   // the default (k = R) is no rule
    if (n_dead && (threadIdx.x & 63u) == 0u && dead) atomicAdd(n_dead, uint32_t(__popcll(dead)));
}

}  // namespace

hipError_t launch_cover_expand(const CoverTile& t, bool k16, void* src, void* dst, uint16_t* dport, uint8_t* proto,
                               int n_cu, hipStream_t s) {
    if (!t.n) return hipSuccess;
    const int grid = reach_grid((uint64_t(t.n) + 3) / 4, 256, n_cu);
    if (k16) hipLaunchKernelGGL(cover_expand16, dim3(grid), dim3(256), 0, s, t, src, dst, dport, proto);
    else hipLaunchKernelGGL(cover_expand4, dim3(grid), dim3(256), 0, s, t, src, dst, dport, proto);
    return hipGetLastError();
}

hipError_t launch_cover_fold(unsigned long long c0, uint32_t n, const uint32_t* rule, uint32_t n_out,
                             unsigned long long* minc, unsigned long long* cnt, int n_cu, hipStream_t s) {
    if (!n) return hipSuccess;
    // at least one step of 256 cells per wave; at most two workgroups per CU
    const int grid = int(std::max<uint64_t>(1, std::min<uint64_t>((uint64_t(n) + kReachChunk - 1) / kReachChunk,
                                                                  uint64_t(std::max(1, n_cu)) * 2)));
    if (n_out <= kCoverBins)
        hipLaunchKernelGGL(cover_fold_bins, dim3(grid), dim3(kReachBlock), size_t(n_out) * 4, s, c0, n, rule, n_out, minc,
                           cnt);
    else
        hipLaunchKernelGGL(cover_fold, dim3(grid), dim3(kReachBlock), 0, s, c0, n, rule, n_out, minc, cnt);
    return hipGetLastError();
}

hipError_t launch_cover_finish(const CoverTile& t, const unsigned long long* minc, uint32_t n_out, uint8_t* live_out,
                               uint4* witness, uint32_t* n_dead, hipStream_t s) {
    hipLaunchKernelGGL(cover_finish, dim3((n_out + 255u) / 256u), dim3(256), 0, s, t, minc, n_out, live_out, witness,
                       n_dead);
    return hipGetLastError();
}

}  // namespace cls
