// Device code shared by the reachability matrix's units (k_reach.hip,
// k_reach_diff.hip, k_reach_ports.hip, k_reach_hops.hip): a tile's cell
// arithmetic (kernels.hpp ReachTile), the wave sum and OR, and the launches'
// grid.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.hpp"

namespace cls {

// Cell i of the tile: row = rows after the tile's first (probe, source) row,
// d = its destination.  One 32-bit division per lane; the lane's following
// cells advance by carries.
struct ReachCell {
    uint32_t row, d;
};
__device__ __forceinline__ ReachCell reach_cell(const ReachTile& t, uint32_t i) {
    const uint32_t x = t.d0 + i;                 // < 2^18 + 2^30
    const uint32_t row = x / t.n_ep;
    return {row, x - row * t.n_ep};
}
// (probe, source) of a row of the tile, relative to the tile's first probe
struct ReachRow {
    uint32_t p, s;
};
__device__ __forceinline__ ReachRow reach_row(const ReachTile& t, uint32_t row) {
    const uint32_t y = t.s0 + row;
    const uint32_t p = y / t.n_ep;
    return {p, y - p * t.n_ep};
}

// sum over the wave's 64 lanes
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// OR over the wave's 64 lanes of a 64-bit word
__device__ __forceinline__ unsigned long long wave_or64(unsigned long long v) {
    uint32_t lo = uint32_t(v), hi = uint32_t(v >> 32);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo |= __shfl_xor(lo, o, 64);
        hi |= __shfl_xor(hi, o, 64);
    }
    return (unsigned long long)hi << 32 | lo;
}

// memory-bound, grid-stride: at most 8 workgroups per CU
inline int reach_grid(uint64_t work, uint32_t per_block, int n_cu) {
    const uint64_t blocks = (work + per_block - 1) / per_block;
    return int(std::max<uint64_t>(1, std::min<uint64_t>(blocks, uint64_t(std::max(1, n_cu)) * 8)));
}

}  // namespace cls
