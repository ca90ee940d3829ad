// Launch interface of the gfx950 kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "compile.hpp"

namespace cls {

// IPv4 packet batch in device memory (structure of arrays)
struct Pkts4 {
    const uint32_t* src;
    const uint32_t* dst;
    const uint16_t* dport;
    const uint8_t* proto;
    uint64_t n;
};

// 16-byte packet batch: network-order addresses (IPv4-mapped = IPv4 packet)
struct Pkts16 {
    const uint4* src;          // 16-B aligned
    const uint4* dst;
    const uint16_t* dport;
    const uint8_t* proto;
    uint64_t n;
    uint32_t vec;              // dport 8-B, proto and verdict 4-B aligned: 4 packets per lane
};

// 16-byte front end (Cls16Image): per side (0 src, 1 dst) the key array's
// and the rep array's LDS byte offsets and the padded key count
struct Fe16 {
    uint32_t key[2], val[2], top[2];
    uint32_t k8[2];            // 8-B keys (compile.hpp key8)
    uint32_t src_mode;         // 1: host-route hashes -> class row (Cls16Image)
    uint32_t h4, cap4, mul4, s4_0, s4_1, L4;             // IPv4-mapped hash (s0 = 32 - L, s1 = 32 - 2 L)
    uint32_t k6, r6, cap6, mul6, s6_0, s6_1, L6, fold[3]; // IPv6 hash
    uint32_t dflt4, dflt6;     // rows of the families' sources no prefix covers
    const uint8_t* gsrc;       // src_mode 1, 2: the source interval table in global memory
    uint32_t gval;             // (keys at 0, reps at gval; gtop keys, 8 B when gk8)
    uint32_t gtop, gk8;
};

struct Cls4Dev {
    const uint32_t* img;       // classifier image (device)
    uint32_t img_bytes;
    uint32_t off_bounds, off_iclass, off_cells, off_lists, off_tmpl;
    uint32_t search_top;       // power of two; bounds padded to 2*search_top
    uint32_t n_ctr;            // slot counters in the image's LDS tail
    uint32_t lds_bytes;
    const LinRule4* lin;       // linear rules (the 16-byte kernel's FORCE_LINEAR cross-check)
    uint32_t n_lin;
    uint32_t n_rules;          // R
    uint32_t mode;             // 0 interval search, 1 hash LPM, 4 source trie
    uint32_t off_trie, trie_depth;   // mode 4: level 1 at off_trie (compile.cpp build_trie)
    const uint8_t* gcells;     // list modes 5, 6: wide cells (uint2 {pointer table, counter base})
    uint32_t default_row;      // source lookup miss: byte address of the default class's cells
    uint32_t n_hash;
    uint32_t hash_mask[kMaxHashLens], hash_shift[kMaxHashLens], hash_cap[kMaxHashLens];
    uint32_t off_hash[kMaxHashLens];
    uint32_t hash_mul[kMaxHashLens], hash_shift1[kMaxHashLens];   // shift1 = 32 - 2 L
    uint32_t list_mode;        // 0 template scan, 1 bit vectors, 2 + global port classes,
                               // 3 port-filtered sublists, 4 + hashed port classes
    uint32_t bv_steps;         // bit-vector search depth (max over lists, both dims)
    uint32_t n_hot;            // slots [0, n_hot) are counted in per-lane LDS rows
    uint32_t off_hot;          // byte offset of the rows (n_hot x 64 u32) in LDS
    uint32_t off_ptop;         // list mode 2: port radix
    uint32_t bv_wide;          // some list > 16 entries: result bits need the hi word
    uint32_t row_bytes;        // cells per class row x cell size (interval search scales by it)
    uint32_t port_mul, port_mask4, port_dflt;   // list mode 4: port perfect hash at LDS 0
    uint32_t n_lctr;           // LDS-resident image: slots [0, n_lctr) counted in LDS, the rest in gslot
    uint32_t ctr16;            // LDS counters are u16 (compile.hpp counter tiers)
    uint32_t* part;            // LDS-resident image: per-workgroup slot counters [grid][n_lctr]
    uint32_t* oq;              // OTHER queue {fill per wave, a segment of oq_cap indices per wave}
                               // (null: classify such packets in place)
    uint32_t oq_cap;
    unsigned long long* zero = nullptr;   // the call's rule counters, cleared by the launch's
    uint32_t n_zero = 0;                  // workgroups before the finish launch adds to them
};

// Whether the classify dispatchers have a kernel for an image of source
// lookup `mode` and `list_mode`, LDS-resident or not; rep16: the 16-byte
// core (mode 3 = rows from the front end's host-route hashes).  The source
// trie and the wide cells exist only in LDS.
inline bool cls_kernel_exists(uint32_t mode, uint32_t list_mode, bool lds, bool rep16) {
    if (list_mode > 6 || (list_mode >= 5 && !lds)) return false;
    switch (mode) {
    case 0: case 1: return true;
    case 3: return rep16;
    case 4: return lds && list_mode >= 3;
    default: return false;
    }
}

struct LaunchCfg {
    int grid;                  // workgroups (persistent, grid-stride)
    hipStream_t stream;
    Cls4Dev other;             // classify kernels: the OTHER image (protocols > 2), global memory
    // classify kernels: events stamped with the kernel's own start / stop
    // (hipExtLaunchKernel: part of the dispatch, no marker packets between
    // kernels); null: none
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
};

// verdict may be null; gslot: u64 slot counters (added to)
hipError_t launch_classify4_cls(const Cls4Dev& t, const Pkts4& p, uint8_t* verdict,
                                unsigned long long* gslot, bool lds_resident, bool vec,
                                const LaunchCfg& cfg);
// lin: linear first match over the rep-space rules (t.lin) after the front end
hipError_t launch_classify16_cls(const Cls4Dev& t, const Fe16& fe, const Pkts16& p, uint8_t* verdict,
                                 unsigned long long* gslot, bool lds_resident, bool lin,
                                 const LaunchCfg& cfg);
// rule_out (not null): each packet's terminating rule (R: the default DENY)
// instead of counting into gslot
hipError_t launch_classify4_linear(const LinRule4* rules, uint32_t n_lin, uint32_t n_rules,
                                   const Pkts4& p, uint8_t* verdict, unsigned long long* gslot,
                                   const LaunchCfg& cfg, uint32_t* rule_out = nullptr);
// slot-mode words (result | slot << 2) -> verdict (may be null) and
// slot_rule[slot] per packet; rule may alias words
hipError_t launch_slot_rules(const uint32_t* words, const uint32_t* slot_rule, uint32_t n, uint8_t* verdict,
                             uint32_t* rule, hipStream_t s);
// slot_val[i] += sum_w part[w * n + i], w < rows (the classify kernel's
// partials); zero[0, n_zero) = 0 in the same launch (zero may be null)
hipError_t launch_fold(const uint32_t* part, uint32_t rows, uint32_t n, unsigned long long* slot_val,
                       unsigned long long* zero, uint32_t n_zero, hipStream_t s);
// out[csr[k].y] += slot_val[csr[k].x], then slot_val[csr[k].x] = 0, for k < n
// (csr: every slot once, grouped by rule); out null: clear only
hipError_t launch_remap(unsigned long long* slot_val, const uint2* csr, uint32_t n, unsigned long long* out,
                        hipStream_t s);
// The end of a classify call, one launch: tiles of 64 slots fold the
// workgroups' LDS partials (part, rows x n_lctr; null: none) and, with
// remap, move slot_val + partials to the rule counters out (slot -> rule:
// slot_rule, entries kHotRule | h for the hot rules -- rules with many slots,
// summed per tile in LDS -- then their n_hot rule ids) and clear slot_val;
// without remap (an earlier chunk of a long batch) slot_val += partials.
// out must be cleared before (the classify launch's zero).
constexpr uint32_t kOtherSegs = 16;   // OTHER queue segments per classify workgroup (its waves)
constexpr uint32_t kHotRule = 0x80000000u;
constexpr uint32_t kMaxHotRules = 64;
struct FinishArgs {
    const uint32_t* part;
    uint32_t rows, n_lctr;
    unsigned long long* slot_val;
    uint32_t n_slots;
    const uint32_t* slot_rule;
    uint32_t n_hot;
    unsigned long long* out;
    bool remap;
    // the OTHER queue of the classify launch (null: none): oq_rows (its
    // workgroups) x kOtherSegs fills, then as many segments of oq_cap
    // entries, one per classify wave; blocks after the tiles classify a
    // workgroup's queued packets (protocols > 2) on the OTHER image and count
    // them per rule -- other_map: compact rule index of each of the n_other
    // OTHER slots, then the n_orules rules
    const uint32_t* oq;
    uint32_t oq_rows, oq_cap;
    uint32_t qmask = 0;          // entries are (packet >> 2) | mask << 28: the packets 4 g + q of the
                                 // mask's bits (IPv4 launches: one entry per lane and wave step)
    const uint32_t* other_map;
    uint32_t n_other, n_orules;
    uint32_t split = 1;          // blocks per tile of 64 slots, each folding a share of the rows
                                 // (remap with partials only; the host's fold_split)
};
// finish4 / finish16: the OTHER packets' loads from the 4- / 16-byte batch
hipError_t launch_finish4(const FinishArgs& f, const Cls4Dev& o, const Pkts4& p, uint8_t* verdict, hipStream_t s);
hipError_t launch_finish16(const FinishArgs& f, const Cls4Dev& t, const Cls4Dev& o, const Fe16& fe, const Pkts16& p,
                           uint8_t* verdict, hipStream_t s);
// the classify kernels' packet stream without the lookups (stream floor);
// exactly one of p4 / p16; p4 needs 16-B aligned src/dst, 8-B dport, 4-B
// proto and verdict (variant bit 0: load and use instead of the next step's
// loads in flight; bit 1: the protocol stream a cached load, not
// non-temporal); p16 covers whole 256-packet wave steps only
hipError_t launch_stream(const Pkts4* p4, const Pkts16* p16, uint8_t* verdict, int grid, int variant,
                         hipStream_t s);

// Slot mode of the classify kernels (connection batches): out[i] = result |
// slot << 2 (u32), no counting; protocols > 2 in place, their slots after
// the main image's.  p4: one packet per lane (no vector requirements).
hipError_t launch_classify4_slots(const Cls4Dev& t, const Pkts4& p, uint32_t* out, bool lds_resident,
                                  const LaunchCfg& cfg);
hipError_t launch_classify16_slots(const Cls4Dev& t, const Fe16& fe, const Pkts16& p, uint32_t* out,
                                   bool lds_resident, const LaunchCfg& cfg);
// The pair image's slot -> rule map as u16 (map, n16 16-B units), staged at
// LDS byte srl after the image (0: none; the launch reads slot_rule)
struct PairMap {
    const uint16_t* map = nullptr;
    uint32_t srl = 0, n16 = 0;
};
// Both tuples of a connection batch in one launch (LDS-resident IPv4 image):
// out[i] = the SYN tuple (p.src, p.dst, p.dport) and out[stride + i] the
// SYN-ACK tuple (p.dst, p.src, sport), result | slot << 2 each.  The OTHER
// image (o, offsets rebased to LDS byte o_at) is staged beside the main one
// when o_at != 0; with o_late (o_at 0, offsets image-relative) it is staged
// at LDS 0, over the main image, once every wave of the workgroup has left
// its main loop.  Connections of protocol > 2 go to the wave's queue
// segment -- lq_cap entries in the LDS after the images, then oq_cap in oq
// (segment w of the grid's waves) -- and are classified on the OTHER image
// after the wave's main loop, one per lane (in place when the segment is
// full, from global memory unless the image sits beside the main one).
// cdiv != 0 (ceil(2^32 / t.row_bytes)): the OTHER image's source classes are
// t's, so a queued connection carries its two classes and the drain skips
// the OTHER source search.  o4: t is the pair image (compile.hpp
// Cls4Opts::with_other, four cells per class): protocols > 2 are classified
// with the others -- no queue, no OTHER image, slots of t's own.
// Needs 16-B aligned src / dst / out / out + stride, 8-B dport / sport, 4-B
// proto; stride a multiple of 4.
// slot_rule (may be null): write each word's counter index ctr_base +
// slot_rule[slot] in place of the slot (counting connection batches).
// wbytes: 4 -- u32 words (SYN at out[i], SYN-ACK at out[stride + i]); 2 --
// u16 words (counter indices < 2^14), the two in one u32 at out[i] (SYN |
// SYN-ACK << 16: one load for the connection kernel); 1 -- only
// the two ACLActions, one byte per connection (SYN result | SYN-ACK result
// << 2) at byte i (batches that do not count)
hipError_t launch_classify4_pair(const Cls4Dev& t, const Cls4Dev& o, uint32_t o_at, const Pkts4& p,
                                 const uint16_t* sport, uint32_t* out, uint64_t stride, uint32_t* oq,
                                 uint32_t oq_cap, const uint32_t* slot_rule, uint32_t ctr_base, uint32_t wbytes,
                                 uint32_t lq_cap, bool o_late, uint32_t cdiv, bool o4, const PairMap& sm,
                                 const LaunchCfg& cfg);
// LDS byte offset of the pair launch's queue segments: after the main image,
// the OTHER image beside it (o_at != 0), or the larger of the two (o_late)
inline uint32_t pair_queue_lds(uint32_t img_bytes, uint32_t o_at, uint32_t o_bytes, bool o_late) {
    const uint32_t end = o_at ? o_at + o_bytes : o_late && o_bytes > img_bytes ? o_bytes : img_bytes;
    return (end + 15u) & ~15u;
}
// The OTHER queue segment of one pair-launch workgroup (kPairBlock threads)
// that holds every connection its lanes visit, 4 per lane per step, in 16-B
// entries; the engine caps the segment (oq_cap entries; the overflow is
// classified in place)
constexpr int kPairBlock = 1024;
inline uint64_t pair_queue_words(uint64_t n, int grid) {
    const uint64_t nsteps = n / 4, nthreads = uint64_t(grid) * kPairBlock;
    return 4ull * kPairBlock * ((nsteps + nthreads - 1) / nthreads);
}

// Both tuples of a 16-byte connection batch in one launch (k16_pair.hip) on
// the table's pair image (compile.hpp build_pair16: four cells per class,
// LDS-resident, no wide cells; fe: its front end): the SYN tuple (p.src,
// p.dst, p.dport) and the SYN-ACK tuple (p.dst, p.src, sport), written as
// launch_classify4_pair writes them (out, stride, slot_rule, ctr_base,
// wbytes, sm as there; slots are the pair image's own).  A destination-keyed
// image takes p.src and p.dst exchanged.  Needs 16-B aligned src / dst, 4-B
// aligned out, p.n <= 2^28 (32-bit byte offsets into the address arrays).
// Whole wave-steps of 64 x kPair16Conns connections take the vector path
// (lane l of a wave: base + 64 k + l), the rest a per-connection tail.
constexpr uint32_t kPair16Conns = 2;   // connections per lane per step
// ... and whether it has a variant for a core of source lookup `mode` and
// `list_mode` behind source front end `src_mode` (Cls16Image): list modes
// 0-4 (an image with wide cells, 5 and 6, never takes the launch)
inline bool pair16_kernel_exists(uint32_t mode, uint32_t list_mode, uint32_t src_mode) {
    if (list_mode > 4 || src_mode > 2) return false;
    if (src_mode) return mode == 3;
    return mode == 0 || mode == 1 || (mode == 4 && list_mode >= 3);
}
hipError_t launch_classify16_pair(const Cls4Dev& t, const Fe16& fe, const Pkts16& p, const uint16_t* sport,
                                  uint32_t* out, uint64_t stride, const uint32_t* slot_rule, uint32_t ctr_base,
                                  uint32_t wbytes, const PairMap& sm, const LaunchCfg& cfg);

struct ConnDesc {                // one bound ACL for the connection kernel
    uint32_t rule_off;           // linear ACLs: first rule in the call's rule pool
    uint32_t n;                  // linear rules
    uint32_t n_rules;            // R (default DENY: rule R)
    uint32_t ctr_off;            // counting: counter of rule 0 in the call's counter space
    int32_t pre_blk;             // classifier slot words' block in ConnArgs::pre (-1: none)
    uint32_t pad;
    const uint32_t* slot_rule;   // pre_blk >= 0: slot -> rule index
    uint32_t bm_off;             // bitmap form (IPv4): byte offset of its tables in the pool; ~0u: none
    uint32_t bm_sd;              // bitmap form: source | destination interval counts << 16
    uint32_t bm_tu;              // bitmap form: TCP | UDP port interval counts << 16
    uint32_t bm_w;               // bitmap form: u32 words per row
};
struct IfAcls {                  // interface -> (inbound, outbound) ConnDesc index, -1 = nil
    int32_t in, out;
    int32_t in_pre, out_pre;     // their classifier slot words' block in ConnArgs::pre (-1: none)
};
static_assert(sizeof(ConnDesc) == 48 && sizeof(IfAcls) == 16, "connect_kernel reads the staged tables as 16-B words");
// The bitmap form of a linear IPv4 ACL in the connection pool (engine.cpp
// conn_bitmap4), u32 words from a 16-B aligned base: header {W, ns, nd, nr,
// n0, n1, n2, n3} (its counts also in the ACL's ConnDesc), then the src
// table {ns keys, ns x W row words}, the dst table, the four protocol tables
// (TCP, UDP by destination port; ICMP and OTHER one row each: n2 = n3 = 1),
// then nr {meta, index} pairs.  Keys are the starts of
// the elementary intervals (key 0 first); a row has bit i set when pool
// rule i matches that interval's addresses (ports); the first match is the
// lowest set bit of src row & dst row & protocol row.
constexpr uint32_t kConnBmHeader = 32;
// Connection counting: the call counters come in kConnCtrCopies copies, so
// that the workgroups' end-of-launch adds to a popular counter spread over
// that many addresses (same-address device atomics serialise); the scatter
// launch sums the copies.  LDS counters are u16 pairs: a workgroup takes at
// most kConnWgConns connections per launch (4 calls each stay below 2^16).
// Connection batches with at most this many large ACLs load every one's
// result words together with the connection's fields (no second dependent
// global round trip behind the interface lookup).
// The connection kernel's state-machine table: one byte per (4 call
// results, same interface, unknown interface).
constexpr uint32_t kConnStateEntries = 1024;
constexpr uint32_t kConnEarlyBlocks = 2;
constexpr uint32_t kConnCtrCopies = 16;
constexpr uint32_t kConnWgConns = 16383;
__host__ __device__ constexpr uint32_t conn_lds_ctr_bytes(uint32_t n_ctr) { return (n_ctr + 1u) / 2u * 4u; }

struct ConnArgs {
    const ConnDesc* desc;
    const IfAcls* ifs;
    uint32_t n_ifs;
    const void* rules;           // ConnRule4 / ConnRule16 pool (global memory)
    uint32_t rules_bytes;        // staged into LDS at address 0 when the launch says so
    uint32_t n_ctr;              // counting: counter space (sum of R + 1 over the descriptors)
    uint32_t ctr_lds;            // counting: LDS byte offset of the counters (LDS variant; u16
                                 // pairs: counter j in half j & 1 of word j >> 1, a workgroup
                                 // evaluates at most kConnWgConns connections per launch)
    uint32_t sm_lds;             // LDS byte offset of the state machine's table (kConnStateEntries B)
    uint32_t ctr16;              // counting, LDS variant: u16 counter pairs (else u32 counters)
    uint32_t* ctr_rows;          // counting, LDS variant: workgroup b stores its LDS counter words
                                 // as row b (null: device atomics into the copies of ctr)
    unsigned long long* ctr;     // counting: the call's u64 counters, kConnCtrCopies copies of
                                 // n_ctr (workgroup b adds to copy b % kConnCtrCopies)
    const uint32_t* src_if;
    const uint32_t* dst_if;
    const void* src;             // u32 host order, or 16-B network-order addresses
    const void* dst;
    const uint16_t* sport;
    const uint16_t* dport;
    const uint8_t* proto;
    uint64_t n;
    uint8_t* out;
    uint32_t n_desc;             // descriptors in desc
    uint32_t meta_lds;           // LDS byte offset of the staged desc + ifs tables; ~0u: global reads
    const uint32_t* pre;         // classifier slot words of the large ACLs: block b at pre + 2 b pre_stride
                                 // (SYN tuple, then SYN-ACK at + pre_stride); null when there are none
    uint64_t pre_stride;
    uint32_t n_big;              // blocks at pre (the large ACLs); <= kConnEarlyBlocks: every block's
                                 // words loaded with the connection's fields, before the interfaces
    uint32_t pre_rules;          // the words carry counter indices (descriptor base + rule), not slots
    uint32_t pre_bytes;          // the words' width: 4; 2 (u16 counter-index words, both tuples'
                                 // in one u32 per connection, SYN | SYN-ACK << 16, block b at
                                 // pre + b pre_stride); 1 (block b is one byte per
                                 // connection at (uint8_t*) pre + b pre_stride: SYN result |
                                 // SYN-ACK result << 2, batches that do not count)
    uint32_t bm_steps;           // bitmap forms: lower-bound steps of the largest interval table
    uint32_t job_lds;            // IPv4: LDS byte offset of the waves' job lists (512 B per wave)
    int32_t* rule_out;           // the trace variant (launch_connect count 3): 4 rules per
                                 // connection, 16-B aligned (last: the other fields' offsets stay)
};
// k16: 16-byte addresses; lds_rules: stage the pool; count: 0 none, 1 LDS
// counters, 2 global (wave-aggregated) counters, 3 no counters but the calls'
// terminating rules to a.rule_out (cls_connect_rules); grid: persistent workgroups
// of `block` threads (512, 768 or 1024); lds: dynamic LDS bytes (pool, LDS
// counters, a.meta_lds tables)
hipError_t launch_connect(const ConnArgs& a, bool k16, bool lds_rules, int count, int grid, int block, size_t lds,
                          hipStream_t s);
// the connection batch's stream without the evaluation (whole 4-connection
// groups of an IPv4 batch; 16-B aligned src / dst / src_if / dst_if, 8-B
// ports, 4-B proto and out)
hipError_t launch_stream_conn(const ConnArgs& a, int grid, hipStream_t s);
// tables' connection counters += the call's counters (ConnDesc ctr_off ..
// + n_rules), which are cleared: a workgroup per descriptor and 256
// counters (max_rules: the largest n_rules of the descriptors)
// rows of the LDS counter words (n_rows rows of nw words; ctr16: u16 pairs)
// -> the tables' connection counters (descriptor d's counters start at
// desc[d].ctr_off, ascending), summed kConnRowsPerSlab rows per thread
constexpr uint32_t kConnRowsPerSlab = 64;
hipError_t launch_conn_rows(const uint32_t* rows, uint32_t n_rows, uint32_t nw, bool ctr16, uint32_t n_ctr,
                            const ConnDesc* desc, uint32_t n_desc, unsigned long long* const* table_ctr,
                            hipStream_t s);
// the call counters (n_slabs copies of n_ctr u64, summed; clear: zero what
// was read) -> the tables' connection counters
hipError_t launch_conn_scatter(const ConnDesc* desc, unsigned long long* const* table_ctr, uint32_t n_desc,
                               uint32_t max_rules, unsigned long long* call_ctr, uint32_t n_slabs, bool clear,
                               uint32_t n_ctr, hipStream_t s);

// ---- the reachability matrix (k_reach.hip; contivcls.h cls_reach_matrix) --
// One tile of the matrix: connections [0, n) of the tile are the cells from
// (p0, s0, d0) on in (probe, source, destination) order, the destination
// varying fastest, over N endpoints.  Every index the kernels form is 32-bit:
// n <= 2^30, N <= 2^18, and the host passes the outputs offset to the tile's
// first probe and row.
struct ReachTile {
    uint32_t n_ep;               // N
    uint32_t p0, s0, d0;         // the tile's first cell
    uint32_t n;                  // connections in the tile (none past the matrix's end)
};
// The tile's connections written as a device batch's arrays (cls_conn_soa):
// four consecutive connections per lane -- 16-B stores to src / dst (one per
// address with 16-byte addresses) / src_if / dst_if, 8-B to the ports, 4-B to
// the protocols; the arrays hold whole groups of four (the connections past n
// of the last group repeat the last one).  ep_if: N interface ids; ep_addr:
// N u32 or N 16-B addresses; probe: P x {sport | dport << 16, proto}.
struct ReachExpand {
    const uint32_t* ep_if;
    const void* ep_addr;
    const uint2* probe;
    uint32_t *src_if, *dst_if;
    void *src, *dst;
    uint16_t *sport, *dport;
    uint8_t* proto;
};
hipError_t launch_reach_expand(const ReachTile& t, const ReachExpand& x, bool k16, int n_cu, hipStream_t s);
// The tile's ConnectionActions summed: hist[4 p' + action] += connections
// (hist at the tile's first probe, or null), allow[r'] += the row's
// CLS_CONN_ALLOW cells (allow at the tile's first (probe, source) row, or
// null).  verdict: the tile's n bytes, 4-B aligned.  A workgroup histograms
// kReachChunk connections at a time in LDS (the chunk's first kReachLdsProbes
// probes; later ones straight to global memory) and adds each non-zero bin
// once; a wave whose 256 connections lie in one row adds its count once.
constexpr uint32_t kReachBlock = 1024, kReachChunk = 4 * kReachBlock, kReachLdsProbes = 64;
hipError_t launch_reach_reduce(const ReachTile& t, const uint8_t* verdict, unsigned long long* hist,
                               uint32_t* allow, int n_cu, hipStream_t s);

// ---- the reachability diff (k_reach_diff.hip; contivcls.h cls_reach_diff) -
// A tile's new verdicts against its baseline bytes (both n bytes, 4-B
// aligned; a cell is changed when the bytes differ), in three launches whose
// order comes from a scan -- no workgroup waits for another.  Chunks are the
// kReachChunk cells a workgroup of reach_reduce takes at a time.
// count: chunk_count[chunk] = the chunk's changed cells (or null);
// trans[16 p' + 4 (base & 3) + (now & 3)] += cells (trans at the tile's first
// probe, or null; binned in LDS like reach_reduce's histogram); changed[r'] +=
// the row's changed cells (changed at the tile's first (probe, source) row,
// or null).  A workgroup takes a run of consecutive chunks (at most two
// workgroups per CU) and adds its bins when a chunk starts in another probe.
hipError_t launch_reach_diff_count(const ReachTile& t, const uint8_t* base, const uint8_t* now, uint32_t* chunk_count,
                                   unsigned long long* trans, uint32_t* changed, int n_cu, hipStream_t s);
// scan (one workgroup): chunk_base[chunk] = *total + the changed cells of the
// tile's earlier chunks; then *total += the tile's changed cells.
hipError_t launch_reach_diff_scan(uint32_t n, const uint32_t* chunk_count, unsigned long long* chunk_base,
                                  unsigned long long* total, hipStream_t s);
// emit: the tile's changed cells as records {probe, src, dst, was | now << 8}
// (cls_reach_change, one 16-B store each) at changes[chunk_base[chunk] + the
// cell's rank in its chunk], while that index is below cap (changes may be
// null: nothing is emitted).  store: null, or where the tile's new bytes go
// (the in-place call's matrix; only words that differ are written).
hipError_t launch_reach_diff_emit(const ReachTile& t, const uint8_t* base, const uint8_t* now,
                                  const uint32_t* chunk_count, const unsigned long long* chunk_base, uint4* changes,
                                  unsigned long long cap, uint8_t* store, int n_cu, hipStream_t s);

// ---- the reachability port sweep (k_reach_ports.hip; contivcls.h cls_reach_ports)
// One tile of the sweep: rows [0, n) are the whole pairs from (s0, d0) on,
// pair-major -- row i is class i % K of pair i / K after the tile's first,
// n = pairs x K <= 2^30.  Every index the kernels form is 32-bit; the host
// passes runs / allow offset to the tile's first pair.  lo: the K class
// starts (ascending, lo[0] == 0); class k is [lo[k], lo[k + 1] - 1], the last
// one ends at 65535.
struct ReachPortsTile {
    uint32_t n_ep;               // N
    uint32_t s0, d0;             // the tile's first pair
    uint32_t K;                  // classes per pair
    uint32_t n;                  // rows in the tile
    const uint16_t* lo;
};
// The tile's rows as a device batch's arrays, in reach_expand's store shape
// (four rows per lane, the last group padded by repetition): dport = lo[k],
// sport and proto constant.
struct ReachPortsExpand {
    const uint32_t* ep_if;
    const void* ep_addr;
    uint32_t sport, proto;
    uint32_t *src_if, *dst_if;
    void *src, *dst;
    uint16_t *sport_out, *dport_out;
    uint8_t* proto_out;
};
hipError_t launch_reach_ports_expand(const ReachPortsTile& t, const ReachPortsExpand& x, bool k16, int n_cu,
                                     hipStream_t s);
// A row starts a range when k == 0 or its verdict byte differs from the row
// before.  count: chunk_count[chunk] = the starts among the chunk's
// kReachChunk rows (or null); runs[pair'] += the pair's starts; allow[pair']
// += width(k) of the rows with CLS_CONN_ALLOW; hist[action] += width(k)
// (binned in LDS, each non-zero bin added once per chunk); each may be null.
// verdict: the tile's n bytes, 4-B aligned.
hipError_t launch_reach_ports_count(const ReachPortsTile& t, const uint8_t* verdict, uint32_t* chunk_count,
                                    uint32_t* runs, uint32_t* allow, unsigned long long* hist, int n_cu,
                                    hipStream_t s);
// emit (behind launch_reach_diff_scan of the chunk counts): the record of the
// range with index j = chunk_base[chunk] + its start's rank in the chunk
// (cls_port_range) while j < cap.  The start row writes src, dst, port_lo and
// the action word; the range's last row -- whose index is the starts up to
// and including it, less one -- writes port_hi; a range of one row takes one
// 16-B store.  No range crosses a tile, so every record below min(total,
// cap) is complete when the launch ends.
hipError_t launch_reach_ports_emit(const ReachPortsTile& t, const uint8_t* verdict,
                                   const unsigned long long* chunk_base, uint4* ranges, unsigned long long cap,
                                   int n_cu, hipStream_t s);

// ---- the external sweep (k_reach_ext.hip; contivcls.h cls_reach_external) --
// One tile of the sweep: rows [0, n) are the whole lines from (dir index d0,
// probe p0, endpoint s0) on, line-major -- row i is class i % K of line i / K
// after the tile's first, lines numbered (d P + p) N + s, n = lines x K <=
// 2^30.  Every index the kernels form is 32-bit: the host passes runs / allow
// offset to the tile's first line and hist to its first (dir, probe).  lo: the
// K class starts (ascending, lo[0] == 0); class k is [lo[k], lo[k + 1] - 1],
// the last one ends at 2^32 - 1, so a width may be 2^32: widths and their
// sums are 64-bit.  dir_of: the direction (0 egress, 1 ingress) of dir index
// 0 and 1.
struct ReachExtTile {
    uint32_t n_ep, n_probes;     // N, P
    uint32_t d0, p0, s0;         // the tile's first line
    uint32_t K;                  // classes per line
    uint32_t n;                  // rows in the tile
    uint32_t dir_of[2];
    const uint32_t* lo;
};
// The tile's rows as a device batch's arrays, in reach_expand's store shape
// (four rows per lane, the last group padded by repetition): the pod side from
// the endpoint table, the remote side ext_if and lo[k] (16-byte layout:
// ::ffff:lo[k]), source and destination by the line's direction, the ports and
// the protocol of the line's probe (P x {sport | dport << 16, proto}).
struct ReachExtExpand {
    const uint32_t* ep_if;
    const void* ep_addr;
    const uint2* probe;
    uint32_t ext_if;
    uint32_t *src_if, *dst_if;
    void *src, *dst;
    uint16_t *sport, *dport;
    uint8_t* proto;
};
hipError_t launch_reach_ext_expand(const ReachExtTile& t, const ReachExtExpand& x, bool k16, int n_cu,
                                   hipStream_t s);
// A row starts a range when k == 0 or its verdict byte differs from the row
// before.  count: chunk_count[chunk] = the starts among the chunk's
// kReachChunk rows (or null); runs[line'] += the line's starts; allow[line']
// += width(k) of the rows with CLS_CONN_ALLOW; hist[4 q' + action] += width(k)
// (q': (dir, probe) after the tile's first); each may be null.  A wave whose
// 256 rows lie in one line adds its sums once, a workgroup whose chunk lies in
// one (dir, probe) bins the histogram in LDS and adds each non-zero bin once.
// verdict: the tile's n bytes, 4-B aligned.
hipError_t launch_reach_ext_count(const ReachExtTile& t, const uint8_t* verdict, uint32_t* chunk_count,
                                  uint32_t* runs, unsigned long long* allow, unsigned long long* hist, int n_cu,
                                  hipStream_t s);
// emit (behind launch_reach_diff_scan of the chunk counts): the record of the
// range with index j = chunk_base[chunk] + its start's rank in the chunk
// (cls_addr_range: {src, probe | dir << 16 | action << 24, addr_lo, addr_hi})
// while j < cap.  The start row writes the first three words, the range's
// last row addr_hi at the same index; a range of one row takes one 16-B
// store.  No range crosses a tile, so every record below min(total, cap) is
// complete when the launch ends.
hipError_t launch_reach_ext_emit(const ReachExtTile& t, const uint8_t* verdict, const unsigned long long* chunk_base,
                                 uint4* ranges, unsigned long long cap, int n_cu, hipStream_t s);

// ---- the rule coverage sweep (k_cover.hip; contivcls.h cls_table_cover) ----
// One tile of the sweep: the n <= 2^30 cells from global cell c0 on, cell c =
// (s Kd + d) T + j (source class s, destination class d, column j), up to 2^40
// of them in all.  slo / dlo: the class starts (ascending, [0] == 0); col: the
// T columns as dport | proto << 16.
struct CoverTile {
    unsigned long long c0;
    uint32_t n;
    uint32_t Kd, T;
    const uint32_t *slo, *dlo, *col;
};
// The tile's cells as a device classify batch's arrays, in reach_expand's
// store shape (four cells per lane, the last group padded by repetition: the
// arrays hold (n + 3) / 4 whole groups): each cell's lowest packet -- the
// class starts (16-byte layout: ::ffff:a), the column's protocol and port.
hipError_t launch_cover_expand(const CoverTile& t, bool k16, void* src, void* dst, uint16_t* dport, uint8_t* proto,
                               int n_cu, hipStream_t s);
// rule: the tile's n terminating rules (16-B aligned), each below n_out = R + 1.
// minc[r] = min(minc[r], the least global cell c0 + i with rule[i] == r);
// cnt[r] += the cells with rule r.  Runs of equal rules reduce in the wave,
// then across the workgroup's waves, before any global atomic.
// Up to 15,360 rules the counts pass through per-workgroup LDS bins
// (cover_fold_bins), above that the run heads add to cnt directly.
hipError_t launch_cover_fold(unsigned long long c0, uint32_t n, const uint32_t* rule, uint32_t n_out,
                             unsigned long long* minc, unsigned long long* cnt, int n_cu, hipStream_t s);
// Once per call, over the n_out rules (t: the class tables; c0 and n unused):
// minc[k] == ~0: dead -- live 0, an all-zero witness, and one more in *n_dead
// (cleared before) when k < R; else live 1 and the witness {src, dst, dport |
// proto << 16 | 1 << 24, 0} of the cell.  live_out, witness, n_dead may be null.
hipError_t launch_cover_finish(const CoverTile& t, const unsigned long long* minc, uint32_t n_out, uint8_t* live_out,
                               uint4* witness, uint32_t* n_dead, hipStream_t s);

// ---- the table diff (k_tdiff.hip; contivcls.h cls_table_diff) --------------
// One tile of the diff: t is a CoverTile over the JOINT classes of the two
// tables whose c0 is a multiple of T and whose n is a whole number of rows of T
// cells (n + T < 2^32); Ks, Kt, Ku complete the dimensions (column j < Kt: TCP,
// j < Kt + Ku: UDP, then the ICMP column and the one of every other protocol).
struct TDiffTile {
    CoverTile t;
    uint32_t Ks, Kt, Ku;
};
// The tile's cells under table a (was, rule_a) and table b (now, rule_b): n
// verdict bytes and n terminating rules each, 16-B aligned.
struct TDiffCells {
    const uint8_t *was, *now;
    const uint32_t *rule_a, *rule_b;
};
// count: a cell differs when was != now.  pairs[4 (was & 3) + (now & 3)] += the
// cells, *n_diff += the differing ones (either may be null), *first = min(*first,
// the least differing global cell); mask_a[i] = rule_a[i] where cell i differs
// and none_a where not, mask_b likewise (what launch_cover_fold reduces per
// rule with n_out = none + 1); chunk_count[chunk] = the run heads of the chunk's
// kReachChunk cells (or null).  A run: a maximal stretch of differing cells of
// one row and one protocol with equal (was, now, rule_a, rule_b).  Ballots in
// the wave, 16 LDS bins per workgroup, one global add per non-zero bin.
hipError_t launch_tdiff_count(const TDiffTile& q, const TDiffCells& c, uint32_t none_a, uint32_t none_b,
                              uint32_t* mask_a, uint32_t* mask_b, uint32_t* chunk_count, unsigned long long* pairs,
                              unsigned long long* n_diff, unsigned long long* first, int n_cu, hipStream_t s);
// emit (behind launch_reach_diff_scan of the chunk counts): the record of the
// run whose head is the chunk's k-th at rec[2 (chunk_base[chunk] + k)], two 16-B
// stores (cls_tdiff_rec), while that index is below cap.
hipError_t launch_tdiff_emit(const TDiffTile& q, const TDiffCells& c, const uint32_t* chunk_count,
                             const unsigned long long* chunk_base, uint4* rec, unsigned long long cap, int n_cu,
                             hipStream_t s);

// ---- the rule necessity sweep (k_need.hip; contivcls.h cls_table_need) -----
// The sweep's tables.  slo / dlo / col: cover's class tables.  bits: the bit
// rows, one bit per rule (bit r & 63 of word r >> 6), W = max(1, (R + 63) / 64)
// u64 words per row, each section's start rounded up to a whole 16 B: S[Ks]
// at word 0, D[Kd] at word wD, C[T] at wC, the kept row (~skip, tail bits
// clear) at wK.  res: one byte per rule, two ACLAction bits per protocol
// (TCP, UDP, ICMP, every other value), [R] zero for the default DENY.
struct NeedTab {
    uint32_t Ks, Kd, T, W, R;
    uint32_t wD, wC, wK;
    const uint32_t *slo, *dlo, *col;
    unsigned long long* bits;
    const uint8_t* res;
};
// The reduced rule's tests of a class start and of a column: what a bit of an
// S, D or C row says (host and device: cls_table_need_host builds the same rows).
__host__ __device__ inline bool need_src_hit(const LinRule4& l, uint32_t a) { return (a & l.src_mask) == l.src_addr; }
__host__ __device__ inline bool need_dst_hit(const LinRule4& l, uint32_t a) { return (a & l.dst_mask) == l.dst_addr; }
__host__ __device__ inline bool need_col_hit(const LinRule4& l, uint32_t col) {
    const uint32_t p = col >> 16 & 3u, w = l.port[p];
    return (l.meta >> (8u * p) & 0x80u) && (col & 0xFFFFu) - (w & 0xFFFFu) <= w >> 16;
}
__host__ __device__ inline uint8_t need_res_byte(uint32_t meta) {
    return uint8_t((meta & 3u) | (meta >> 8 & 3u) << 2 | (meta >> 16 & 3u) << 4 | (meta >> 24 & 3u) << 6);
}
// The S, D and C rows from the n_lin reduced rules (ascending LinRule4::index
// below R; a rule absent from the list sets no bit): one thread per output
// word, 64 rule tests each.  The kept row is the caller's.
hipError_t launch_need_bits(const NeedTab& q, const LinRule4* lin, uint32_t n_lin, hipStream_t s);
// One tile of whole (s, d) pairs: `pairs` of them from pair0 = s Kd + d on,
// tile cell i = (pair - pair0) T + j (pairs T < 2^32).  One wave per pair; the
// column rows in LDS when cols_lds (the caller checked that T W 8 bytes fit
// need_cols_lds_max()).  need == null, the first pass: first[i] = first(c),
// mark[i] = first(c) where the cell changes under it, R + 1 where not.
// need != null (the R need bytes), the second pass: mark[i] = first(c) where
// second(c) is a rule that is not CLS_NEED_NEEDED, R + 1 elsewhere; first
// unused.  Both arrays are what launch_cover_fold reduces with n_out = R + 2.
hipError_t launch_need_cells(const NeedTab& q, unsigned long long pair0, uint32_t pairs, const uint8_t* need,
                             uint32_t* first, uint32_t* mark, bool cols_lds, int n_cu, hipStream_t s);
uint32_t need_cols_lds_max();
// Once per call over the R rules: need[r] from the kept row and the two count
// rows (cells with first == r, cells changing under r); counts[need[r]] += 1
// (cleared before; or null); changed[r] = cnt_chg[r] (or null).
hipError_t launch_need_mark(const NeedTab& q, const unsigned long long* cnt_first, const unsigned long long* cnt_chg,
                            uint8_t* need, uint32_t* counts, unsigned long long* changed, hipStream_t s);
// free[r] = DEAD, or REDUNDANT with no chained cell.
hipError_t launch_need_free(uint32_t R, const uint8_t* need, const unsigned long long* cnt_chain, uint8_t* free_out,
                            hipStream_t s);
// Rule r's least changing cell min_chg[r] -> its witness {src, dst, dport |
// proto << 16 | (0x80 | after) << 24, fall}, second recomputed for that one
// cell; zeros for a rule that is not CLS_NEED_NEEDED.
hipError_t launch_need_finish(const NeedTab& q, const unsigned long long* min_chg, const uint8_t* need, uint4* witness,
                              hipStream_t s);

// ---- the hop closure (k_reach_hops.hip; contivcls.h cls_reach_hops) --------
// fold: the tile's CLS_CONN_ALLOW cells off the diagonal as bits of the
// adjacency bitmap adj[N][W], W = (N + 63) / 64 -- bit (d & 63) of word
// s W + (d >> 6), whatever the cell's probe (the union over probes).  verdict:
// the tile's n bytes (no alignment needed).  A wave takes 64 consecutive
// cells, builds each touched word from a ballot and ORs it in once.
hipError_t launch_reach_adj_fold(const ReachTile& t, const uint8_t* verdict, unsigned long long* adj, int n_cu,
                                 hipStream_t s);
// bfs: the level-synchronous breadth-first search from every source over adj,
// at most max_hops (1 .. 254) levels.  A workgroup owns `rows` (4, 8 or 16)
// consecutive source rows from level 1 to the end, their reached / frontier /
// next bit rows in LDS, and writes their outputs, each of which may be null:
// hops[s N + d] (every byte once: 0 on the diagonal, the level, or 255),
// reach[s], closure[s W + w]; it adds to exposed[d] and levels[256], which
// the caller cleared.  No workgroup waits for another.
constexpr uint32_t kHopsBlock = 256;
size_t reach_hops_lds(uint32_t n_ep, uint32_t rows);      // the launch's LDS bytes
uint32_t reach_hops_rows(uint32_t n_ep, uint32_t want);   // want (0: 4, the measured best) cut to what fits LDS
hipError_t launch_reach_hops_bfs(uint32_t n_ep, uint32_t max_hops, uint32_t rows, const unsigned long long* adj,
                                 uint8_t* hops, uint32_t* reach, uint32_t* exposed, unsigned long long* levels,
                                 unsigned long long* closure, hipStream_t s);

// ---- the reachability classes (k_reach_classes.hip; contivcls.h cls_reach_classes)
// fold: per cell (p, s, d) off the diagonal of the tile, sums[(p N + s) 2] +=
// class_g(seed_r, p, d, value) and sums[(p N + d) 2 + 1] += class_g(seed_c, p,
// s, value) (reach_classes.hpp; 64-bit, wrapping: the values do not depend on
// the order); diag[p N + s] = the diagonal cell; mask[8]: bit v set for every
// byte v of the tile.  sums and mask: cleared by the caller before the first
// tile; all three are the whole matrix's (p counts from the matrix's first
// probe).  verdict: the tile's n bytes (no alignment needed).
hipError_t launch_reach_class_fold(const ReachTile& t, const uint8_t* verdict, uint64_t seed_r, uint64_t seed_c,
                                   unsigned long long* sums, uint8_t* diag, uint32_t* mask, hipStream_t s);
// verify: every cell of the tile against tab[P][n_classes][n_classes + 1]
// (reach_classes.hpp: the entry of (p, cls[s], s == d ? n_classes : cls[d]);
// cleared to empty by the caller before the first tile); *bad |= 1 on a
// mismatch.  cls: the N candidate classes, each < n_classes.
hipError_t launch_reach_class_verify(const ReachTile& t, const uint8_t* verdict, const uint32_t* cls, uint32_t n_classes,
                                     uint32_t* tab, uint32_t* bad, hipStream_t s);

struct TrafficDev {
    uint64_t seed;
    uint32_t pct_pod, pct_dst, pct_port, pct_icmp;
    const uint32_t* pods; uint32_t n_pods;
    const uint32_t* dst_addrs; const uint8_t* dst_lens; uint32_t n_dst;
    const uint16_t* ports; uint32_t n_ports;
};
hipError_t launch_gen4(const TrafficDev& t, uint64_t first, uint64_t n, uint32_t* src,
                       uint32_t* dst, uint16_t* sport, uint16_t* dport, uint8_t* proto,
                       hipStream_t s);

// 16-byte stream (contivcls.h cls_traffic_spec16); pools as (hi, lo) u64 pairs
struct TrafficDev16 {
    uint64_t seed;
    uint32_t pct_pod, pct_dst, pct_port, pct_icmp;
    const uint64_t* pods; uint32_t n_pods;
    const uint64_t* dst_addrs; const uint8_t* dst_lens; uint32_t n_dst;
    const uint16_t* ports; uint32_t n_ports;
};
hipError_t launch_gen16(const TrafficDev16& t, uint64_t first, uint64_t n, uint4* src, uint4* dst,
                        uint16_t* sport, uint16_t* dport, uint8_t* proto, hipStream_t s);

int max_lds_bytes();             // per-workgroup LDS the classify kernel may use
int cls_block();                 // classify workgroup size

}  // namespace cls
