// The reachability diff's kernels (kernels.hpp; reach.cpp cls_reach_diff): a
// tile's new verdicts against its baseline bytes.  reach_diff_count counts
// the changed cells of every chunk, the transitions per probe and the changed
// cells per (probe, source) row; reach_diff_scan turns the chunk counts into
// each chunk's first record index behind the call's running total;
// reach_diff_emit writes the records there -- an ordered stream compaction
// whose order comes from the scan alone.  Plain C++ throughout: vector
// stores, LDS and global atomics.
#include <hip/hip_runtime.h>

#include "k_reach_dev.hpp"
#include "kernels.hpp"

namespace cls {

namespace {

constexpr uint32_t kWaves = kReachBlock / 64u;
static_assert(16u * kReachLdsProbes == kReachBlock, "one transition bin per thread");

// The lane's four cells: base and new bytes (one 4-B load each; the matrix's
// last, partial group byte by byte: nothing is read past the tile), x their
// difference -- a byte of x is non-zero where the cell changed, and zero past
// the tile.
struct DiffWords {
    uint32_t b4, v4, x, live;
};
__device__ __forceinline__ DiffWords diff_load(const ReachTile& t, const uint8_t* base, const uint8_t* now,
                                               uint32_t i0) {
    DiffWords w{0u, 0u, 0u, 0u};
    if (i0 + 4u <= t.n) {
        w.b4 = *reinterpret_cast<const uint32_t*>(base + i0);
        w.v4 = *reinterpret_cast<const uint32_t*>(now + i0);
        w.live = 4u;
    } else if (i0 < t.n) {
        w.live = t.n - i0;
        for (uint32_t k = 0; k < w.live; ++k) {
            w.b4 |= uint32_t(base[i0 + k]) << (8u * k);
            w.v4 |= uint32_t(now[i0 + k]) << (8u * k);
        }
    }
    w.x = w.b4 ^ w.v4;
    return w;
}
__device__ __forceinline__ uint32_t byte_of(uint32_t w, uint32_t k) { return (w >> (8u * k)) & 0xFFu; }

// The workgroup's transition bins, of probes pb on, added to trans and cleared
// (behind a barrier; nothing was added to them without trans).
__device__ __forceinline__ void flush_bins(uint32_t* bins, unsigned long long* trans, uint32_t pb) {
    const uint32_t b = bins[threadIdx.x];
    if (b) {
        atomicAdd(&trans[16ull * pb + threadIdx.x], (unsigned long long)b);
        bins[threadIdx.x] = 0u;
    }
}

__global__ __launch_bounds__(kReachBlock) void reach_diff_count(ReachTile t, const uint8_t* base, const uint8_t* now,
                                                                uint32_t* chunk_count, unsigned long long* trans,
                                                                uint32_t* changed) {
    __shared__ uint32_t bins[16u * kReachLdsProbes];
    __shared__ uint32_t n_changed;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t chunks = (t.n + kReachChunk - 1u) / kReachChunk;
    bins[threadIdx.x] = 0u;                                        // (each flush clears them again)
    if (threadIdx.x == 0u) n_changed = 0u;
    __syncthreads();
    // a workgroup takes consecutive chunks, so that its bins -- of probes
    // [pb, pb + kReachLdsProbes) -- reach global memory once per probe it
    // starts a chunk in, not once per chunk: the adds of all workgroups go to
    // the same few words
    const uint32_t per = (chunks + gridDim.x - 1u) / gridDim.x;
    const uint32_t ch_a = min(blockIdx.x * per, chunks), ch_b = min(ch_a + per, chunks);
    uint32_t pb = 0u;
    for (uint32_t ch = ch_a; ch < ch_b; ++ch) {
        const uint32_t c0 = ch * kReachChunk;                      // the chunk's first cell
        const uint32_t pc = reach_row(t, reach_cell(t, c0).row).p; // its first probe
        if (ch == ch_a) pb = pc;
        if (pc != pb) {                                            // workgroup-uniform
            flush_bins(bins, trans, pb);
            __syncthreads();
            pb = pc;
        }
        const uint32_t i0 = c0 + 4u * threadIdx.x;                 // the lane's four cells
        const uint32_t w0 = i0 - 4u * lane;                        // the wave's 256
        if (w0 < t.n) {                                            // wave-uniform
            const uint32_t wl = min(w0 + 255u, t.n - 1u);
            const uint32_t row_a = reach_cell(t, w0).row, row_b = reach_cell(t, wl).row;
            const uint32_t p_a = reach_row(t, row_a).p, p_b = reach_row(t, row_b).p;
            const DiffWords w = diff_load(t, base, now, i0);
            uint32_t wc = 0u;                                      // the wave's changed cells, <= 256
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) wc += __popcll(__ballot(byte_of(w.x, k) != 0u));
            if (chunk_count && lane == 0u && wc) atomicAdd(&n_changed, wc);
            if (changed && wc) {
                if (row_a == row_b) {
                    if (lane == 0u) atomicAdd(&changed[row_a], wc);
                } else {
                    // a wave across rows: each lane adds its cells' runs per row
                    ReachCell c = reach_cell(t, i0 < t.n ? i0 : w0);
                    uint32_t run = 0u;
                    for (uint32_t k = 0; k < w.live; ++k) {
                        run += byte_of(w.x, k) ? 1u : 0u;
                        if (++c.d == t.n_ep || k + 1u == w.live) {
                            if (run) atomicAdd(&changed[c.row], run);
                            run = 0u;
                            c.d = 0;
                            ++c.row;
                        }
                    }
                }
            }
            if (trans) {
                if (p_a == p_b) {
                    // the lane's counts per transition 4 (base & 3) + new, u8
                    // fields of acc[base & 3]; summed over each half of the
                    // wave (<= 128 per field), whose lanes 0..15 add one
                    // transition each
                    uint32_t acc[4] = {0u, 0u, 0u, 0u};
                    for (uint32_t k = 0; k < w.live; ++k) {
                        const uint32_t a = byte_of(w.b4, k) & 3u, one = 1u << (8u * (byte_of(w.v4, k) & 3u));
#pragma unroll
                        for (uint32_t j = 0; j < 4u; ++j) acc[j] += a == j ? one : 0u;
                    }
#pragma unroll
                    for (int o = 16; o > 0; o >>= 1) {
#pragma unroll
                        for (uint32_t j = 0; j < 4u; ++j) acc[j] += __shfl_xor(acc[j], o, 64);
                    }
                    const uint32_t f = lane & 15u;
                    const uint32_t r = f < 4u ? acc[0] : f < 8u ? acc[1] : f < 12u ? acc[2] : acc[3];
                    const uint32_t c = byte_of(r, f & 3u);
                    if ((lane & 31u) < 16u && c) {
                        if (p_a - pb < kReachLdsProbes) atomicAdd(&bins[16u * (p_a - pb) + f], c);
                        else atomicAdd(&trans[16ull * p_a + f], (unsigned long long)c);
                    }
                } else {
                    ReachCell c = reach_cell(t, i0 < t.n ? i0 : w0);
                    ReachRow r = reach_row(t, c.row);
                    for (uint32_t k = 0; k < w.live; ++k) {
                        const uint32_t f = 4u * (byte_of(w.b4, k) & 3u) + (byte_of(w.v4, k) & 3u);
                        if (r.p - pb < kReachLdsProbes) atomicAdd(&bins[16u * (r.p - pb) + f], 1u);
                        else atomicAdd(&trans[16ull * r.p + f], 1ull);
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
        }
        __syncthreads();
        if (threadIdx.x == 0u) {
            if (chunk_count) chunk_count[ch] = n_changed;
            n_changed = 0u;
        }
        __syncthreads();                                           // before the next chunk's adds
    }
    flush_bins(bins, trans, pb);
}

// One workgroup: thread i takes the counts [i per, (i + 1) per); an inclusive
// scan of the threads' sums in LDS gives each its first index.
__global__ __launch_bounds__(kReachBlock) void reach_diff_scan(uint32_t n, const uint32_t* chunk_count,
                                                               unsigned long long* chunk_base,
                                                               unsigned long long* total) {
    __shared__ unsigned long long part[kReachBlock];
    const unsigned long long before = *total;                      // read by all before the barriers, written after
    const uint32_t per = (n + kReachBlock - 1u) / kReachBlock;
    const uint32_t a = min(threadIdx.x * per, n), b = min(a + per, n);
    unsigned long long sum = 0ull;
    for (uint32_t i = a; i < b; ++i) sum += chunk_count[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t o = 1u; o < kReachBlock; o <<= 1) {
        const unsigned long long v = threadIdx.x >= o ? part[threadIdx.x - o] : 0ull;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long at = before + part[threadIdx.x] - sum;
    for (uint32_t i = a; i < b; ++i) {
        chunk_base[i] = at;
        at += chunk_count[i];
    }
    if (threadIdx.x == kReachBlock - 1u) *total = before + part[threadIdx.x];
}

__global__ __launch_bounds__(kReachBlock) void reach_diff_emit(ReachTile t, const uint8_t* base, const uint8_t* now,
                                                               const uint32_t* chunk_count,
                                                               const unsigned long long* chunk_base, uint4* changes,
                                                               unsigned long long cap, uint8_t* store) {
    __shared__ uint32_t wave_n[kWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t chunks = (t.n + kReachChunk - 1u) / kReachChunk;
    for (uint32_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        // workgroup-uniform: a chunk without a changed cell, or whose records
        // all lie past cap, has nothing to write
        if (!chunk_count[ch]) continue;
        const unsigned long long first = chunk_base[ch];
        const bool emit = changes && first < cap;
        if (!emit && !store) continue;
        const uint32_t i0 = ch * kReachChunk + 4u * threadIdx.x;   // the lane's four cells
        const DiffWords w = diff_load(t, base, now, i0);
        if (store && w.x) {
            if (w.live == 4u) *reinterpret_cast<uint32_t*>(store + i0) = w.v4;
            else
                for (uint32_t k = 0; k < w.live; ++k) store[i0 + k] = uint8_t(byte_of(w.v4, k));
        }
        if (!emit) continue;
        // the changed cells before the lane's in its wave (cell order: the
        // lower lanes' cells come first), and the wave's
        uint32_t below = 0u, mine = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const unsigned long long m = __ballot(byte_of(w.x, k) != 0u);
            below += __popcll(m & ((1ull << lane) - 1ull));
            mine += __popcll(m);
        }
        if (lane == 0u) wave_n[wave] = mine;
        __syncthreads();
        unsigned long long at = first + below;
        for (uint32_t k = 0; k < wave; ++k) at += wave_n[k];
        if (w.x) {
            ReachCell c = reach_cell(t, i0);
            ReachRow r = reach_row(t, c.row);
            for (uint32_t k = 0; k < w.live; ++k) {
                if (byte_of(w.x, k)) {
                    if (at < cap)
                        changes[at] = uint4{t.p0 + r.p, r.s, c.d, byte_of(w.b4, k) | byte_of(w.v4, k) << 8};
                    ++at;
                }
                if (++c.d == t.n_ep) {
                    c.d = 0;
                    if (++r.s == t.n_ep) {
                        r.s = 0;
                        ++r.p;
                    }
                }
            }
        }
        __syncthreads();                                           // before the next chunk's wave counts
    }
}

}  // namespace

hipError_t launch_reach_diff_count(const ReachTile& t, const uint8_t* base, const uint8_t* now, uint32_t* chunk_count,
                                   unsigned long long* trans, uint32_t* changed, int n_cu, hipStream_t s) {
    if (!t.n || (!chunk_count && !trans && !changed)) return hipSuccess;
    // two workgroups of kReachBlock fill a CU: no more, so that each has a long run of chunks
    const int grid = std::min(reach_grid(t.n, kReachChunk, n_cu), 2 * std::max(1, n_cu));
    hipLaunchKernelGGL(reach_diff_count, dim3(grid), dim3(kReachBlock), 0, s, t, base, now, chunk_count, trans,
                       changed);
    return hipGetLastError();
}

hipError_t launch_reach_diff_scan(uint32_t n, const uint32_t* chunk_count, unsigned long long* chunk_base,
                                  unsigned long long* total, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(reach_diff_scan, dim3(1), dim3(kReachBlock), 0, s, n, chunk_count, chunk_base, total);
    return hipGetLastError();
}

hipError_t launch_reach_diff_emit(const ReachTile& t, const uint8_t* base, const uint8_t* now,
                                  const uint32_t* chunk_count, const unsigned long long* chunk_base, uint4* changes,
                                  unsigned long long cap, uint8_t* store, int n_cu, hipStream_t s) {
    if (!t.n || (!changes && !store)) return hipSuccess;
    const int grid = reach_grid(t.n, kReachChunk, n_cu);
    hipLaunchKernelGGL(reach_diff_emit, dim3(grid), dim3(kReachBlock), 0, s, t, base, now, chunk_count, chunk_base,
                       changes, cap, store);
    return hipGetLastError();
}

}  // namespace cls
