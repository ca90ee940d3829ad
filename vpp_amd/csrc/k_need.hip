// The rule necessity sweep's kernels (kernels.hpp NeedTab; need.cpp
// cls_table_need).  In the reduced form of the rules "rule k terminates packet
// x" is a conjunction of three tests -- the source class, the destination
// class, the (protocol, port class) column -- so with one bit per rule the set
// of ALL rules that would take cell (s, d, j) is S[s] & D[d] & C[j] & kept: its
// lowest set bit is the first match, the next one the rule that takes over
// when the first is deleted.  need_bits builds the rows; need_cells walks the
// cells, one wave per (s, d) pair, and writes the u32 arrays cover_fold
// (k_cover.hip) reduces per rule; need_mark, need_free and need_finish run once
// per call over the R rules.  Nothing waits on another workgroup.  Plain C++
// throughout: vector stores, LDS, ballots before global atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "../../include/contivcls.h"
#include "k_reach_dev.hpp"
#include "kernels.hpp"

namespace cls {

namespace {

constexpr uint32_t kCellsBlock = 1024;                    // need_cells: sixteen waves, a pair each, one LDS copy of the column rows
constexpr uint32_t kCellsWaves = kCellsBlock / 64u;
constexpr uint32_t kColsLdsMax = 144u * 1024u;            // of the CU's 160 KiB; one workgroup per CU above 80 KiB
constexpr int kRegWords = 4;                              // words of a pair's row per lane in registers: R <= 16,384

// ---- need_bits -----------------------------------------------------------
// Thread idx = w rows + row (the row fastest: a wave's lanes share w, so the
// rule loads are wave-uniform and each rule is tested against 64 rows at once).
__global__ __launch_bounds__(256) void need_bits(NeedTab q, const LinRule4* __restrict__ lin, uint32_t n_lin) {
    const uint32_t rows = q.Ks + q.Kd + q.T;
    const uint64_t idx = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (idx >= uint64_t(rows) * q.W) return;
    const uint32_t w = uint32_t(idx / rows), row = uint32_t(idx - uint64_t(w) * rows);
    // the first reduced rule with index >= 64 w
    uint32_t lo = 0, hi = n_lin;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (lin[mid].index < 64u * w) lo = mid + 1u;
        else hi = mid;
    }
    const uint32_t kind = row < q.Ks ? 0u : row < q.Ks + q.Kd ? 1u : 2u;
    const uint32_t key = kind == 0u ? q.slo[row] : kind == 1u ? q.dlo[row - q.Ks] : q.col[row - q.Ks - q.Kd];
    unsigned long long word = 0ull;
    for (uint32_t i = lo; i < n_lin; ++i) {
        const LinRule4 l = lin[i];
        if (l.index >= 64u * w + 64u || l.index >= q.R) break;
        const bool hit = kind == 0u ? need_src_hit(l, key) : kind == 1u ? need_dst_hit(l, key) : need_col_hit(l, key);
        if (hit) word |= 1ull << (l.index & 63u);
    }
    const size_t at = kind == 0u   ? size_t(row) * q.W
                      : kind == 1u ? size_t(q.wD) + size_t(row - q.Ks) * q.W
                                   : size_t(q.wC) + size_t(row - q.Ks - q.Kd) * q.W;
    q.bits[at + w] = word;
}

// ---- need_cells ----------------------------------------------------------
__device__ __forceinline__ unsigned long long lane_word(unsigned long long x, uint32_t l) {
    const uint32_t lo = __builtin_amdgcn_readlane(uint32_t(x), l), hi = __builtin_amdgcn_readlane(uint32_t(x >> 32), l);
    return (unsigned long long)hi << 32 | lo;
}

// The first two set bits over the words a stride's lanes hold (word 64 k +
// lane, ascending k then lane = ascending rule): wave-uniform.
struct Two {
    uint32_t first, second, found;
};
__device__ __forceinline__ void two_of_stride(unsigned long long x, uint32_t k, Two& t) {
    unsigned long long b = __ballot(x != 0ull);
    while (b && t.found < 2u) {
        const uint32_t l = uint32_t(__ffsll((long long)b)) - 1u;
        unsigned long long xl = lane_word(x, l);
        const uint32_t base = (64u * k + l) * 64u;
        const uint32_t bit = uint32_t(__ffsll((long long)xl)) - 1u;
        if (t.found == 0u) {
            t.first = base + bit;
            t.found = 1u;
            xl &= xl - 1ull;
            if (xl) {
                t.second = base + uint32_t(__ffsll((long long)xl)) - 1u;
                t.found = 2u;
            }
        } else {
            t.second = base + bit;
            t.found = 2u;
        }
        b &= b - 1ull;
    }
}

// NW > 0: lane l keeps words l, l + 64, ... of S[s] & D[d] & kept in NW
// registers (W <= 64 NW) and per column ANDs in C[j]: nothing but the column
// row is read per cell.  NW == 0, any W: the four rows are read per cell.
// kLds: the column rows were staged in LDS (T W words).
template <int NW, bool kLds>
__global__ __launch_bounds__(kCellsBlock) void need_cells(NeedTab q, unsigned long long pair0, uint32_t pairs,
                                                          const uint8_t* __restrict__ need,
                                                          uint32_t* __restrict__ first_out,
                                                          uint32_t* __restrict__ mark_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long cl[];
    const unsigned long long* __restrict__ Sg = q.bits;
    const unsigned long long* __restrict__ Dg = q.bits + q.wD;
    const unsigned long long* __restrict__ Cg = q.bits + q.wC;
    const unsigned long long* __restrict__ Kg = q.bits + q.wK;
    const uint32_t W = q.W, R = q.R, T = q.T;
    if constexpr (kLds) {
        // the section starts on a 16-B boundary: whole 16-B loads, then the odd last word
        const uint32_t n2 = T * W / 2u;
        for (uint32_t i = threadIdx.x; i < n2; i += blockDim.x)
            reinterpret_cast<uint4*>(cl)[i] = reinterpret_cast<const uint4*>(Cg)[i];
        if ((T * W & 1u) && threadIdx.x == 0u) cl[T * W - 1u] = Cg[T * W - 1u];
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t strides = (W + 63u) / 64u;
    for (uint32_t pair = blockIdx.x * kCellsWaves + wave; pair < pairs; pair += gridDim.x * kCellsWaves) {
        const unsigned long long gp = pair0 + pair;
        const uint32_t s = uint32_t(gp / q.Kd), d = uint32_t(gp - (unsigned long long)s * q.Kd);
        const unsigned long long* Sr = Sg + size_t(s) * W;
        const unsigned long long* Dr = Dg + size_t(d) * W;
        unsigned long long sd[NW > 0 ? NW : 1];
        if constexpr (NW > 0) {
#pragma unroll
            for (int k = 0; k < NW; ++k) {
                const uint32_t wi = lane + 64u * uint32_t(k);
                sd[k] = wi < W ? Sr[wi] & Dr[wi] & Kg[wi] : 0ull;
            }
        }
        const uint32_t base = pair * T;                       // pairs T < 2^32
        // 64 columns at a time: the wave finds each column's first and second
        // (wave-uniform) and lane jj keeps column j0 + jj's; then every lane
        // looks up its own column's result bytes and stores -- no load that
        // depends on a cell's result sits in the serial chain of the columns
        for (uint32_t j0 = 0; j0 < T; j0 += 64u) {
            const uint32_t nj = min(64u, T - j0);
            uint32_t keep_f = R, keep_s = R;
            for (uint32_t jj = 0; jj < nj; ++jj) {
                const uint32_t j = j0 + jj;
                Two t{R, R, 0u};
                if constexpr (NW > 0) {
                    unsigned long long x[NW];
#pragma unroll
                    for (int k = 0; k < NW; ++k) {                      // every stride's word before the first ballot
                        const uint32_t wi = lane + 64u * uint32_t(k);
                        unsigned long long c = 0ull;
                        if (wi < W) c = kLds ? cl[j * W + wi] : Cg[size_t(j) * W + wi];
                        x[k] = sd[k] & c;
                    }
#pragma unroll
                    for (int k = 0; k < NW; ++k)
                        if (t.found < 2u) two_of_stride(x[k], uint32_t(k), t);   // wave-uniform
                } else {
                    for (uint32_t k = 0; k < strides && t.found < 2u; ++k) {
                        const uint32_t wi = lane + 64u * k;
                        unsigned long long x = 0ull;
                        if (wi < W) x = Sr[wi] & Dr[wi] & Kg[wi] & (kLds ? cl[j * W + wi] : Cg[size_t(j) * W + wi]);
                        two_of_stride(x, k, t);
                    }
                }
                if (lane == jj) {
                    keep_f = t.first;
                    keep_s = t.second;
                }
            }
            if (lane < nj) {
                const uint32_t j = j0 + lane;
                uint32_t mark = R + 1u;
                if (keep_f < R) {
                    if (need == nullptr) {
                        const uint32_t sh = 2u * (q.col[j] >> 16 & 3u);
                        if ((q.res[keep_f] >> sh & 3u) != (q.res[keep_s] >> sh & 3u)) mark = keep_f;   // res[R] = DENY
                    } else if (keep_s < R && need[keep_s] != CLS_NEED_NEEDED) {
                        mark = keep_f;
                    }
                }
                if (need == nullptr) first_out[base + j] = keep_f;
                mark_out[base + j] = mark;
            }
        }
    }
}

template <auto K>
void lds_ceiling() {
    // the dynamic-LDS ceiling, raised once per (kernel, device)
    static std::atomic<uint64_t> done{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize,
                              int(kColsLdsMax));
    done.fetch_or(bit, std::memory_order_release);
}

template <int NW, bool kLds>
hipError_t launch_cells(const NeedTab& q, unsigned long long pair0, uint32_t pairs, const uint8_t* need, uint32_t* first,
                        uint32_t* mark, int n_cu, hipStream_t s) {
    const size_t lds = kLds ? size_t(q.T) * q.W * 8u : 0u;
    if constexpr (kLds) lds_ceiling<need_cells<NW, kLds>>();
    // grid-stride over the pairs; the LDS form stages the column rows once per
    // workgroup.  The cells are latency-bound (LDS read, ballot, readlane per
    // column in sequence), so what counts is waves per CU: two workgroups of
    // sixteen fill a CU's 32 wave slots while the rows stay at or below 80 KiB
    const uint32_t per_cu = lds > 80u * 1024u ? 1u : 2u;
    const uint64_t blocks = (uint64_t(pairs) + kCellsWaves - 1u) / kCellsWaves;
    const int grid = int(std::max<uint64_t>(1, std::min<uint64_t>(blocks, uint64_t(std::max(1, n_cu)) * per_cu)));
    hipLaunchKernelGGL((need_cells<NW, kLds>), dim3(grid), dim3(kCellsBlock), lds, s, q, pair0, pairs, need, first,
                       mark);
    return hipGetLastError();
}

template <bool kLds>
hipError_t launch_cells_nw(const NeedTab& q, unsigned long long pair0, uint32_t pairs, const uint8_t* need,
                           uint32_t* first, uint32_t* mark, int n_cu, hipStream_t s) {
    const uint32_t nw = (q.W + 63u) / 64u;
    if (nw <= 1u) return launch_cells<1, kLds>(q, pair0, pairs, need, first, mark, n_cu, s);
    if (nw == 2u) return launch_cells<2, kLds>(q, pair0, pairs, need, first, mark, n_cu, s);
    if (nw <= uint32_t(kRegWords)) return launch_cells<kRegWords, kLds>(q, pair0, pairs, need, first, mark, n_cu, s);
    return launch_cells<0, kLds>(q, pair0, pairs, need, first, mark, n_cu, s);
}

// ---- once per call over the rules ----------------------------------------
__global__ __launch_bounds__(256) void need_mark(NeedTab q, const unsigned long long* __restrict__ cnt_first,
                                                 const unsigned long long* __restrict__ cnt_chg, uint8_t* need,
                                                 uint32_t* counts, unsigned long long* changed) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t v = 4u;                                          // no rule
    if (r < q.R) {
        const bool kept = q.bits[q.wK + (r >> 6)] >> (r & 63u) & 1ull;
        v = !kept ? CLS_NEED_SKIPPED : !cnt_first[r] ? CLS_NEED_DEAD : !cnt_chg[r] ? CLS_NEED_REDUNDANT : CLS_NEED_NEEDED;
        need[r] = uint8_t(v);
        if (changed) changed[r] = kept ? cnt_chg[r] : 0ull;
    }
    if (!counts) return;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        const unsigned long long b = __ballot(v == k);
        if (b && (threadIdx.x & 63u) == 0u) atomicAdd(&counts[k], uint32_t(__popcll(b)));
    }
}

__global__ __launch_bounds__(256) void need_free(uint32_t R, const uint8_t* __restrict__ need,
                                                 const unsigned long long* __restrict__ cnt_chain, uint8_t* free_out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    free_out[r] = need[r] == CLS_NEED_DEAD || (need[r] == CLS_NEED_REDUNDANT && !cnt_chain[r]) ? 1u : 0u;
}

// One thread per rule: the next set bit above r in the rule's least changing
// cell, a serial walk of at most W words.
__global__ __launch_bounds__(256) void need_finish(NeedTab q, const unsigned long long* __restrict__ min_chg,
                                                   const uint8_t* __restrict__ need, uint4* witness) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= q.R) return;
    uint4 out{0u, 0u, 0u, 0u};
    const unsigned long long m = min_chg[r];
    if (need[r] == CLS_NEED_NEEDED && m != ~0ull) {
        const unsigned long long sdi = m / q.T;
        const uint32_t j = uint32_t(m - sdi * q.T);
        const uint32_t s = uint32_t(sdi / q.Kd), d = uint32_t(sdi - (unsigned long long)s * q.Kd);
        const unsigned long long* Sr = q.bits + size_t(s) * q.W;
        const unsigned long long* Dr = q.bits + q.wD + size_t(d) * q.W;
        const unsigned long long* Cr = q.bits + q.wC + size_t(j) * q.W;
        const unsigned long long* Kr = q.bits + q.wK;
        uint32_t fall = q.R;
        for (uint32_t w = r >> 6; w < q.W; ++w) {
            unsigned long long x = Sr[w] & Dr[w] & Cr[w] & Kr[w];
            if (w == r >> 6) x &= (r & 63u) == 63u ? 0ull : ~0ull << ((r & 63u) + 1u);
            if (x) {
                fall = 64u * w + uint32_t(__ffsll((long long)x)) - 1u;
                break;
            }
        }
        const uint32_t col = q.col[j];
        const uint32_t after = q.res[fall] >> (2u * (col >> 16 & 3u)) & 3u;
        out = uint4{q.slo[s], q.dlo[d], (col & 0xFFFFFFu) | (0x80u | after) << 24, fall};
    }
    witness[r] = out;
}

}  // namespace

uint32_t need_cols_lds_max() { return kColsLdsMax; }

hipError_t launch_need_bits(const NeedTab& q, const LinRule4* lin, uint32_t n_lin, hipStream_t s) {
    const uint64_t words = uint64_t(q.Ks + q.Kd + q.T) * q.W;       // below 2^31 words under the cap's 2^20 MiB
    hipLaunchKernelGGL(need_bits, dim3(uint32_t((words + 255u) / 256u)), dim3(256), 0, s, q, lin, n_lin);
    return hipGetLastError();
}

hipError_t launch_need_cells(const NeedTab& q, unsigned long long pair0, uint32_t pairs, const uint8_t* need,
                             uint32_t* first, uint32_t* mark, bool cols_lds, int n_cu, hipStream_t s) {
    if (!pairs) return hipSuccess;
    return cols_lds ? launch_cells_nw<true>(q, pair0, pairs, need, first, mark, n_cu, s)
                    : launch_cells_nw<false>(q, pair0, pairs, need, first, mark, n_cu, s);
}

hipError_t launch_need_mark(const NeedTab& q, const unsigned long long* cnt_first, const unsigned long long* cnt_chg,
                            uint8_t* need, uint32_t* counts, unsigned long long* changed, hipStream_t s) {
    if (!q.R) return hipSuccess;
    hipLaunchKernelGGL(need_mark, dim3((q.R + 255u) / 256u), dim3(256), 0, s, q, cnt_first, cnt_chg, need, counts,
                       changed);
    return hipGetLastError();
}

hipError_t launch_need_free(uint32_t R, const uint8_t* need, const unsigned long long* cnt_chain, uint8_t* free_out,
                            hipStream_t s) {
    if (!R) return hipSuccess;
    hipLaunchKernelGGL(need_free, dim3((R + 255u) / 256u), dim3(256), 0, s, R, need, cnt_chain, free_out);
    return hipGetLastError();
}

hipError_t launch_need_finish(const NeedTab& q, const unsigned long long* min_chg, const uint8_t* need, uint4* witness,
                              hipStream_t s) {
    if (!q.R) return hipSuccess;
    hipLaunchKernelGGL(need_finish, dim3((q.R + 255u) / 256u), dim3(256), 0, s, q, min_chg, need, witness);
    return hipGetLastError();
}

}  // namespace cls
