// The reachability classes' kernels (kernels.hpp; reach.cpp
// cls_reach_classes): reach_class_fold adds a tile's cells into the keyed
// 64-bit row and column sums, reach_class_verify checks a tile's cells against
// the one value of their (probe, class, class) entry.  Plain C++ throughout:
// shuffles, vector stores, LDS and global atomics.  No workgroup
// waits for another, and every loop has a bound of its own.
#include <hip/hip_runtime.h>

#include "k_reach_dev.hpp"
#include "kernels.hpp"
#include "reach_classes.hpp"

namespace cls {

namespace {

using u64 = unsigned long long;

// sum over the wave's 64 lanes of a 64-bit word (wrapping)
__device__ __forceinline__ u64 wave_sum64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The (probe, source) rows of the tile, whole or cut at the tile's ends, in
// bands of kBand: a workgroup takes 256 columns x one band, a thread one
// column d over the band's rows -- no division per cell, one per row.  Cell
// (rr, d) of the tile is byte rr N + d - d0, inside [0, n).
constexpr uint32_t kBand = 64;
__device__ __forceinline__ bool band_cell(const ReachTile& t, uint32_t rr, uint32_t d, long long& i) {
    i = (long long)rr * t.n_ep + d - t.d0;                         // < 2^30 N + N
    return d < t.n_ep && i >= 0 && i < (long long)t.n;
}

// Column sums: a thread owns its column over the band and adds its sum once
// per probe of the band (one atomic per workgroup, column and probe; the other
// shape, one atomic per cell, took 3.6 times as long: DESIGN 5b).  Row sums:
// per row each wave sums its 64 columns and adds once.  The sums wrap mod
// 2^64, so their values do not depend on the order of the adds.  The bytes
// present: bits of an LDS mask, ORed into the global one once per workgroup
// and word.
__global__ __launch_bounds__(256) void reach_class_fold(ReachTile t, uint32_t rows, const uint8_t* verdict, u64 seed_r,
                                                        u64 seed_c, u64* sums, uint8_t* diag, uint32_t* mask) {
    __shared__ uint32_t lmask[8];
    if (threadIdx.x < 8u) lmask[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t d = blockIdx.y * 256u + threadIdx.x;            // the thread's column (< N + 256)
    const uint32_t r0 = blockIdx.x * kBand, r1 = min(rows, r0 + kBand);
    u64 acc = 0ull;                                                // != 0 only with d < N
    uint32_t acc_p = ~0u;
    for (uint32_t rr = r0; rr < r1; ++rr) {                        // at most kBand turns
        const ReachRow r = reach_row(t, rr);
        const uint32_t p = t.p0 + r.p;
        if (acc_p != p) {                                          // (uniform) the band enters another probe
            if (acc) atomicAdd(&sums[(size_t(acc_p) * t.n_ep + d) * 2u + 1u], acc);
            acc = 0ull;
            acc_p = p;
        }
        long long i;
        u64 gr = 0ull;
        if (band_cell(t, rr, d, i)) {
            const uint32_t v = verdict[i];
            if (!((lmask[v >> 5] >> (v & 31u)) & 1u)) atomicOr(&lmask[v >> 5], 1u << (v & 31u));
            if (d == r.s) {
                diag[size_t(p) * t.n_ep + r.s] = uint8_t(v);
            } else {
                gr = class_g(seed_r, p, d, v);
                acc += class_g(seed_c, p, r.s, v);
            }
        }
        const u64 sum = wave_sum64(gr);
        if (lane == 0u && sum) atomicAdd(&sums[(size_t(p) * t.n_ep + r.s) * 2u], sum);
    }
    if (acc) atomicAdd(&sums[(size_t(acc_p) * t.n_ep + d) * 2u + 1u], acc);
    __syncthreads();
    if (threadIdx.x < 8u && lmask[threadIdx.x]) atomicOr(&mask[threadIdx.x], lmask[threadIdx.x]);
}

// Every cell must equal the one value recorded for its (probe, class of s,
// class of d or the diagonal) entry of tab[P][C][C + 1]: the entry is loaded
// first and set by compare-and-swap only while it is empty (an entry never
// changes once set, so a stale empty load only costs the swap, which returns
// the value that won).  Any mismatch raises *bad.  The thread's column keeps
// its class over the band; the row's class and table row are uniform.
__global__ __launch_bounds__(256) void reach_class_verify(ReachTile t, uint32_t rows, const uint8_t* verdict,
                                                          const uint32_t* cls, uint32_t C, uint32_t* tab, uint32_t* bad) {
    const uint32_t d = blockIdx.y * 256u + threadIdx.x;
    const uint32_t r0 = blockIdx.x * kBand, r1 = min(rows, r0 + kBand);
    const uint32_t cd = d < t.n_ep ? cls[d] : 0u;
    bool wrong = false;
    for (uint32_t rr = r0; rr < r1; ++rr) {                        // at most kBand turns
        const ReachRow r = reach_row(t, rr);
        long long i;
        if (!band_cell(t, rr, d, i)) continue;
        const uint32_t want = kClassSet | verdict[i];
        uint32_t* e = tab + (size_t(t.p0 + r.p) * C + cls[r.s]) * (size_t(C) + 1u) + (d == r.s ? C : cd);
        uint32_t have = *e;
        if (have == kClassEmpty) {
            const uint32_t old = atomicCAS(e, kClassEmpty, want);
            have = old == kClassEmpty ? want : old;
        }
        wrong |= have != want;
    }
    if (wrong) atomicOr(bad, 1u);
}

// the launches' grid: bands x blocks of 256 columns
inline dim3 band_grid(const ReachTile& t, uint32_t& rows) {
    rows = uint32_t((uint64_t(t.d0) + t.n + t.n_ep - 1) / t.n_ep);         // <= 2^30 + 1
    return dim3((rows + kBand - 1) / kBand, (t.n_ep + 255u) / 256u);
}

}  // namespace

hipError_t launch_reach_class_fold(const ReachTile& t, const uint8_t* verdict, uint64_t seed_r, uint64_t seed_c,
                                   unsigned long long* sums, uint8_t* diag, uint32_t* mask, hipStream_t s) {
    if (!t.n) return hipSuccess;
    uint32_t rows = 0;
    const dim3 grid = band_grid(t, rows);
    hipLaunchKernelGGL(reach_class_fold, grid, dim3(256), 0, s, t, rows, verdict, u64(seed_r), u64(seed_c), sums, diag,
                       mask);
    return hipGetLastError();
}

hipError_t launch_reach_class_verify(const ReachTile& t, const uint8_t* verdict, const uint32_t* cls, uint32_t n_classes,
                                     uint32_t* tab, uint32_t* bad, hipStream_t s) {
    if (!t.n) return hipSuccess;
    uint32_t rows = 0;
    const dim3 grid = band_grid(t, rows);
    hipLaunchKernelGGL(reach_class_verify, grid, dim3(256), 0, s, t, rows, verdict, cls, n_classes, tab, bad);
    return hipGetLastError();
}

}  // namespace cls
