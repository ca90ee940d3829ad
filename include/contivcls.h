/*
 * contivcls.h -- C ABI of the MI355X batched first-match ACL classifier.
 *
 * This is the drop-in boundary for the Contiv-VPP policy verdict backend.
 * In the reference the verdict backend is the Go test engine
 * mock/aclengine/aclengine_mock.go (MockACLEngine); in production it is VPP's
 * acl-plugin (external C binary, not in the reference tree).  Every entry
 * point below names the reference interface it replaces (file:line relative to
 * the reference root).  A Go (cgo) binding of these entry points is shown in
 * INTEGRATION.md.
 *
 * Conventions
 *  - All functions return 0 (CLS_OK) or a negative CLS_E_* code; the detail is
 *    available from cls_last_error().  Per-packet semantic failures are
 *    VERDICTS (CLS_ACL_FAILURE / CLS_CONN_FAILURE), never error codes.
 *  - The caller owns every buffer.  The engine retains no caller pointer after
 *    a call returns (cgo rule); rule tables are deep-copied by cls_table_put.
 *  - Enum values keep the reference's numeric values.
 *  - IPv4 addresses in the 4-byte SoA are host-order uint32 (a.b.c.d =
 *    a<<24|b<<16|c<<8|d).  16-byte addresses are network-order bytes; an
 *    IPv4-mapped address (::ffff:a.b.c.d) is an IPv4 packet, exactly like Go's
 *    net.IP.To4().
 */
#ifndef CONTIVCLS_H
#define CONTIVCLS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: cls_image_v4_header gained n_lctr, ctr16, swap (a destination-keyed
 *    image: the packets' src and dst must be exchanged) and off_other (a
 *    nested OTHER image); blob version 3; cls_table_info's n_lctr, ctr16,
 *    list_mode and swap; CLS_F_COUNT; CLS_AF_V16 connections;
 *    cls_acl_stats.  A v1 consumer that ignores `swap` would misread blobs. */
/* 4: cls_config's device list (multi-device engines); engine-owned batches
 *    (cls_batch_*); cls_classify_batch / cls_batch_connect; the in-library
 *    RCCL counter all-reduce (cls_comm_*); cls_shard_range. */
/* 5: cls_engine_set_option (tuning / diagnostic switches; the library no
 *    longer reads the process environment); cls_compile_v4 / v16 take an
 *    option string; entry points restore the caller's current device; over
 *    distinct devices an engine without RCCL keeps host-summed counters;
 *    cls_classify_rules (the per-packet matched-rule trace); CLS_F_DEVICE
 *    connection batches are stream-ordered. */
/* 5 (additive): cls_reach_matrix; cls_reach_diff (the changed cells of a
 *    reachability matrix against a baseline: cls_reach_change,
 *    cls_reach_diff_out); cls_reach_ports (per-pair port ranges over all
 *    65,536 destination ports: cls_port_range, cls_reach_ports_out) and
 *    cls_port_classes; cls_reach_hops (the multi-hop closure of the matrix:
 *    hop counts, blast radius, exposure: cls_reach_hops_out, CLS_HOPS_NONE)
 *    and the hops_rows option; cls_reach_classes (the endpoints the matrix
 *    cannot tell apart and the quotient matrix between their classes:
 *    cls_reach_classes_out, CLS_CLASS_NONE), its device-free twin
 *    cls_reach_classes_host and the classes_key_bits option;
 *    cls_reach_external (per-pod remote address ranges over all of IPv4, to
 *    and from the node's output interface: cls_addr_range,
 *    cls_reach_ext_out, CLS_EXT_*) and cls_addr_classes; cls_table_cover
 *    (the rules of one table no packet terminates at and a witness packet
 *    for each of the others: cls_cover_witness, cls_cover_out),
 *    cls_cover_classes and the cover_tile option; cls_table_diff (the packets
 *    whose verdict differs between two tables, as records over the joint
 *    classes, and the rules responsible: cls_tdiff_rec, cls_tdiff_out);
 *    cls_table_need (the rules a table can lose without changing a verdict:
 *    cls_need_witness, cls_need_out, CLS_NEED_*), its device-free twin
 *    cls_table_need_host and the need_bitmap_mb and need_cols_lds options. */
#define CLS_ABI_VERSION 5

/* ---- status codes ------------------------------------------------------ */
enum {
    CLS_OK = 0,
    CLS_E_INVAL = -1,    /* bad argument / malformed rule (would panic in Go) */
    CLS_E_NOMEM = -2,
    CLS_E_HIP = -3,      /* HIP runtime error */
    CLS_E_RCCL = -4,     /* RCCL (the counter all-reduce) unavailable or failed */
    CLS_E_NOTFOUND = -5, /* unknown table / ACL name */
    CLS_E_NODEV = -6     /* no usable gfx950 device */
};

/* ---- reference enums ----------------------------------------------------- */
/* vpp_acl.AclAction (acl.proto:4-8); any other int32 is carried verbatim. */
enum { CLS_ACTION_DENY = 0, CLS_ACTION_PERMIT = 1, CLS_ACTION_REFLECT = 2 };

/* ACLAction returned by evalACL (aclengine_mock.go:63-77). */
enum {
    CLS_ACL_DENY = 0,
    CLS_ACL_PERMIT = 1,
    CLS_ACL_REFLECT = 2,
    CLS_ACL_FAILURE = 3
};

/* ConnectionAction returned by Connection* (aclengine_mock.go:46-60). */
enum {
    CLS_CONN_DENY_SYN = 0,
    CLS_CONN_DENY_SYN_ACK = 1,
    CLS_CONN_ALLOW = 2,
    CLS_CONN_FAILURE = 3
};

/* ProtocolType (aclengine_mock.go:80-91).  Any other value takes evalACL's
 * `switch protocol` fall-through (no case): networks alone decide. */
enum { CLS_PROTO_TCP = 0, CLS_PROTO_UDP = 1, CLS_PROTO_ICMP = 2 };

/* ---- one ACL rule, as the vpp_acl protobuf carries it --------------------
 * Mirrors AccessLists_Acl_Rule (acl.pb.go / acl.proto:17-146).  Presence bits
 * stand for the nil-ness of each protobuf sub-message, because evalACL's
 * semantics depend on it (aclengine_mock.go:481-664).  Networks are the CIDR
 * STRINGS of the protobuf; the engine parses them with Go 1.9 net.ParseCIDR
 * semantics, so a string that fails to parse yields the same FAILURE verdicts
 * the Go engine returns.  NULL or "" means "no network" (match all).
 */
enum {
    CLS_R_MATCHES = 1u << 0,     /* rule.Matches != nil (nil would panic: rejected) */
    CLS_R_MACIP = 1u << 1,       /* Matches.MacipRule != nil */
    CLS_R_IPRULE = 1u << 2,      /* Matches.IpRule != nil */
    CLS_R_IP = 1u << 3,          /* IpRule.Ip != nil */
    CLS_R_OTHER = 1u << 4,       /* IpRule.Other != nil */
    CLS_R_TCP = 1u << 5,         /* IpRule.Tcp != nil */
    CLS_R_TCP_SRC = 1u << 6,     /* Tcp.SourcePortRange != nil */
    CLS_R_TCP_DST = 1u << 7,     /* Tcp.DestinationPortRange != nil */
    CLS_R_UDP = 1u << 8,         /* IpRule.Udp != nil */
    CLS_R_UDP_SRC = 1u << 9,
    CLS_R_UDP_DST = 1u << 10,
    CLS_R_ICMP = 1u << 11,       /* IpRule.Icmp != nil */
    CLS_R_ICMP_CODE = 1u << 12,  /* Icmp.IcmpCodeRange != nil */
    CLS_R_ICMP_TYPE = 1u << 13,  /* Icmp.IcmpTypeRange != nil */
    CLS_R_ICMPV6 = 1u << 14,     /* Icmp.Icmpv6 == true */
    CLS_R_ACTIONS = 1u << 15     /* rule.Actions != nil */
};

typedef struct cls_rule {
    uint32_t flags;             /* CLS_R_* */
    int32_t acl_action;         /* Actions.AclAction (vpp_acl.AclAction) */
    const char* src_network;    /* IpRule.Ip.SourceNetwork */
    const char* dst_network;    /* IpRule.Ip.DestinationNetwork */
    uint32_t tcp_src_lo, tcp_src_hi, tcp_dst_lo, tcp_dst_hi;
    uint32_t udp_src_lo, udp_src_hi, udp_dst_lo, udp_dst_hi;
    uint32_t icmp_code_first, icmp_code_last, icmp_type_first, icmp_type_last;
} cls_rule;

/* ---- packet batches (structure of arrays) -------------------------------- */
enum { CLS_AF_V4 = 4, CLS_AF_V16 = 16 };

typedef struct cls_pkt_soa {
    uint32_t af;               /* CLS_AF_V4: src4/dst4; CLS_AF_V16: src16/dst16 */
    const uint32_t* src4;      /* host-order IPv4 */
    const uint32_t* dst4;
    const uint8_t* src16;      /* n x 16 bytes */
    const uint8_t* dst16;
    const uint16_t* sport;     /* used by the connection path only (SYN-ACK) */
    const uint16_t* dport;
    const uint8_t* proto;      /* ProtocolType */
} cls_pkt_soa;

/* cls_classify / cls_connect_batch flags */
enum {
    CLS_F_DEVICE = 1u << 0,       /* every pointer is device memory on this engine's GPU */
    CLS_F_NO_VERDICT = 1u << 1,   /* verdict_out may be NULL (counters only) */
    CLS_F_ACCUMULATE = 1u << 2,   /* add to counters_out instead of overwriting */
    CLS_F_FORCE_LINEAR = 1u << 3, /* use the linear (ballot) kernel: GPU cross-check */
    CLS_F_TIMING = 1u << 4,       /* record HIP events around the classify kernel */
    CLS_F_CONN_CLS = 1u << 5,     /* cls_connect_batch: use the classifier images at any batch size */
    CLS_F_COUNT = 1u << 6         /* cls_connect_batch: count every evalACL call's terminating rule
                                     into the tables' connection counters (cls_conn_counters) */
};

typedef struct cls_engine cls_engine;

/* An engine over one device (n_devices = 0: `device`) or over several
 * (n_devices > 0: devices[0 .. n_devices), `device` ignored).
 * A multi-device engine keeps one ACL configuration: every table is compiled
 * once and uploaded to every device (replicated), and batches (cls_batch_*)
 * shard contiguously over the devices.  Calls that take raw packet pointers
 * (cls_classify, cls_connect_batch, cls_gen_traffic_*) run on the first
 * device.  Over distinct devices the engine creates an RCCL communicator
 * (single-process ncclCommInitAll) at creation, so batch hit counters merge
 * with an all-reduce over xGMI; a list that repeats a device (diagnostics:
 * shards on one GPU), or a host where RCCL cannot be loaded or initialised,
 * has no communicator and its counters are summed on the host when read
 * (cls_comm_info reports 0 ranks; cls_last_error keeps the RCCL reason). */
typedef struct cls_config {
    int device;                /* HIP device ordinal; -1 = current device */
    uint32_t n_devices;        /* 0: one device (`device`); else the length of `devices` */
    const int* devices;        /* HIP device ordinals (n_devices of them) */
    uint32_t reserved[4];
} cls_config;

/* ---- engine lifetime ---------------------------------------------------- */
/* Replaces NewMockACLEngine (aclengine_mock.go:124).  Destroy batches
 * (cls_batch_destroy) before their engine. */
int cls_engine_create(const cls_config* cfg, cls_engine** out);
void cls_engine_destroy(cls_engine* e);
/* Devices of the engine (1 for a single-device engine). */
int cls_engine_devices(const cls_engine* e, uint32_t* n_devices);
/* The engine of device `index` of a multi-device engine (0: `e` itself):
 * a borrowed handle for the single-device calls on that device (timing,
 * stream floors, raw device pointers of that device); configuration calls on
 * it are refused (configure through `e`). */
int cls_device_engine(cls_engine* e, uint32_t index, cls_engine** dev);
/* The message of the engine's last failing call.  The pointer is the engine's
 * own string: it is valid only until the next failing call on that engine
 * from any thread, which rewrites and may reallocate it.  A caller that
 * shares the engine with other threads goes by the return code and reads the
 * text only where it knows no other call can fail meanwhile. */
const char* cls_last_error(const cls_engine* e);
int cls_abi_version(void);
/* Diagnostics, tests and measurements: one tuning switch of the engine (and
 * of every device of a multi-device engine), `value` NULL for its default.
 * The switches force compiler choices (list_mode, list_mode_max, trie, wide,
 * orient=src|dst, lds_budget, src_search, phash_dense, v16_src_search,
 * v16_src_trie) for later cls_table_put / cls_acl_put compiles, and launch
 * plans (other_cap, wg_per_cu, fold_split, conn_bitmap, conn_pair, conn_pair16, conn_pre_rules,
 * conn_pre_narrow, conn_wg_per_cu, conn_wg768, pair_qcap, pair_lq, pair_other_global,
 * pair_other_late, pair_o4, pair_map_lds, pair_class, conn_no_lds,
 * conn_jobs, conn_plan=32j|16j|32s|16s, conn_flush_atomic, batch_layout,
 * reach_tile -- cls_reach_matrix's connections per tile, 256 .. 2^30, rounded
 * up to a multiple of 1024 --, cover_tile -- cls_table_cover's cells per tile,
 * 1024 .. 2^30, rounded up likewise --, need_bitmap_mb, need_cols_lds, hops_rows, classes_key_bits, debug_modes, debug_conn, debug_floor) for
 * later calls; every one keeps verdicts and counters exact.  The library never reads the environment:
 * an engine runs its defaults unless told otherwise here.  CLS_E_INVAL for
 * an unknown key or a malformed value. */
int cls_engine_set_option(cls_engine* e, const char* key, const char* value);

/* ---- rule tables (one compiled, device-resident ACL) -------------------
 * cls_table_put compiles an ACL's rules (evalACL semantics,
 * aclengine_mock.go:473-668) into the engine's device layout and uploads it.
 * Replaces the per-evaluation re-parse of acl.Rules (aclengine_mock.go:480-524).
 */
int cls_table_put(cls_engine* e, const char* name, const cls_rule* rules,
                  uint32_t n_rules, uint32_t* table_id);
int cls_table_del(cls_engine* e, uint32_t table_id);

typedef struct cls_table_info {
    uint32_t n_rules;          /* R: counters_out has R+1 entries */
    uint32_t kernel;           /* 0 = linear (ballot) kernel, 1 = compiled classifier */
    uint32_t lds_bytes;        /* LDS image of the compiled classifier (v4) */
    uint32_t n_intervals;      /* elementary source intervals (v4) */
    uint32_t n_classes;        /* distinct source-prefix classes (v4) */
    uint32_t n_templates;      /* distinct (dst, port range, result) tuples (v4) */
    uint32_t n_slots;          /* flattened candidate slots (v4) */
    uint32_t lds_resident;     /* 1 if the classifier fits LDS, else global memory */
    uint32_t has_v16;          /* 1 if CLS_AF_V16 batches can be classified */
    uint32_t lds_bytes_v16;    /* LDS image of the 16-byte layout's classifier */
    uint32_t lds_resident_v16;
    uint32_t n_lctr;           /* slots counted in LDS (v4; the rest in global memory) */
    uint32_t ctr16;            /* the LDS slot counters are u16 (v4) */
    uint32_t list_mode;        /* candidate-list mode of the v4 classifier (cls_image_v4_header) */
    uint32_t swap;             /* the v4 classifier is keyed on destinations (cls_image_v4_header) */
    uint32_t reserved[1];
} cls_table_info;
int cls_table_get_info(cls_engine* e, uint32_t table_id, cls_table_info* info);

/* ---- batched first-match -------------------------------------------------
 * verdict_out[i] = evalACL(acl, pkt i) (ACLAction, aclengine_mock.go:473-668).
 * counters_out[k] (k < R) = packets whose evaluation terminated at rule k,
 * counters_out[R] = packets that fell through to the default DENY (:667).
 * `stream` is a hipStream_t (NULL: the engine's own stream).  The call is
 * synchronous with respect to the host unless CLS_F_DEVICE is set, in which
 * case work is only enqueued on `stream`.
 * Threading: any thread may call; calls are serialised while they enqueue.
 * Device work of concurrent calls on different streams may overlap, also on
 * one table: every (table, stream) pair has its own counter scratch.  A
 * table deleted (cls_table_del, cls_acl_put/del) while device work on it is
 * pending is freed only after that work finishes.
 */
int cls_classify(cls_engine* e, uint32_t table_id, const cls_pkt_soa* pkts,
                 uint64_t n, uint8_t* verdict_out, uint64_t* counters_out,
                 uint32_t flags, void* stream);

/* The per-packet trace of evalACL's matched rule (the reference logs it at
 * Debug, aclengine_mock.go:651-654): verdict_out[i] as cls_classify (may be
 * NULL) and rule_out[i] = the index k of the rule at which packet i's
 * evaluation terminated, R for the default DENY (:667) -- the counter
 * cls_classify adds the packet to.  No counters are touched.  Flags:
 * CLS_F_DEVICE (device arrays, rule_out 4-byte aligned; stream-ordered),
 * else host arrays and the call returns with the results.  A table that has
 * no 16-byte classifier (cls_table_info's has_v16 == 0) returns CLS_E_INVAL
 * for a CLS_AF_V16 batch, as cls_classify does.  Replaces, for a batch, the
 * rule index evalACL computes and logs per call. */
int cls_classify_rules(cls_engine* e, uint32_t table_id, const cls_pkt_soa* pkts,
                       uint64_t n, uint8_t* verdict_out, uint32_t* rule_out,
                       uint32_t flags, void* stream);

/* Milliseconds of the last classify kernel (CLS_F_TIMING), measured with HIP
 * events on the launch stream.  Blocks until that kernel has finished.
 * Serialised with the other calls like them: among concurrent timed calls it
 * reports one whole call's pair, the last one enqueued. */
int cls_last_kernel_ms(cls_engine* e, float* ms);
/* Every classify kernel timed (CLS_F_TIMING) since the last reset: up to `cap`
 * durations in launch order; *count = number recorded.  Recording enqueues
 * only events (no host synchronisation); reading blocks until every one has
 * finished (timed calls on several streams finish in any order). */
int cls_kernel_times(cls_engine* e, float* ms, uint32_t cap, uint32_t* count);
/* The same kernels' start times, milliseconds after the first one's: the
 * differences are the launch-to-launch period of a stream of timed calls
 * (each kernel stamps its own start, so no event marker sits between them).
 * Kernels timed on different streams start in any order: launch order, in
 * which both calls list them, is start order on one stream only. */
int cls_kernel_starts(cls_engine* e, float* ms, uint32_t cap, uint32_t* count);
int cls_kernel_times_reset(cls_engine* e);

/* Measurement only (bench.py): the classify kernel's HBM stream without the
 * lookups -- the same loads and stores, order and grid -- over a device batch
 * (CLS_AF_V4: 16-B aligned addresses, 8-B dport, 4-B proto and verdict;
 * CLS_AF_V16: 16-B aligned addresses, whole 256-packet steps), `reps` timed
 * launches after one warm-up; *ms = the average launch.  Writes verdict. */
int cls_stream_floor(cls_engine* e, const cls_pkt_soa* pkts, uint64_t n, uint8_t* verdict,
                     uint32_t reps, float* ms, void* stream);
/* The same, one average per stream shape (cls_stream_floor returns their
 * minimum): shape = variant << 1 | (two 1024-thread workgroups per CU, else
 * one -- the classify kernel's own shape when its LDS image takes more than
 * half of the CU's LDS); variant 0 / 1 / 2 / 3 = loads as classify4_cls / one
 * step ahead / protocol non-temporal / both (CLS_AF_V16: variant 0 only).  Up
 * to `cap` times into ms; *count = the number of shapes. */
int cls_stream_floor_shapes(cls_engine* e, const cls_pkt_soa* pkts, uint64_t n, uint8_t* verdict,
                            uint32_t reps, float* ms, uint32_t cap, uint32_t* count, void* stream);

/* ---- ACL configuration (ACLConfig, aclengine_mock.go:110-121,671-728) --- */
/* PutACL semantics (:699-728): requires >=1 interface; re-putting a name
 * replaces it without counting an extra change; last writer wins per
 * interface direction.  A re-put whose rules equal the installed ACL's (the
 * renderer re-puts a local table whose pods changed, acl_renderer.go:186-190)
 * keeps the compiled table and only moves the interface bindings: no
 * compilation, no upload.  Either way the put installs a new ACL, so its
 * connection counters (cls_conn_counters) start from zero. */
int cls_acl_put(cls_engine* e, const char* acl_name, const cls_rule* rules,
                uint32_t n_rules, const char* const* ingress_ifs, uint32_t n_ingress,
                const char* const* egress_ifs, uint32_t n_egress);
/* DelACL semantics (:680-696). */
int cls_acl_del(cls_engine* e, const char* acl_name);
/* Table id of the installed ACL `acl_name` (GetACLByName, :228-234). */
int cls_acl_table(cls_engine* e, const char* acl_name, uint32_t* table_id);
/* GetNumOfACLs (:209), GetNumOfACLChanges (:237). */
int cls_acl_counts(cls_engine* e, uint32_t* n_acls, uint32_t* n_changes);
/* cls_acl_put calls that compiled a table / that kept the installed one. */
int cls_acl_stats(cls_engine* e, uint32_t* n_compiles, uint32_t* n_rebinds);
/* Interface id used by cls_conn_batch; ids are stable for the engine's life. */
int cls_if_id(cls_engine* e, const char* if_name, uint32_t* id);
/* Table id of the inbound/outbound ACL on an interface, -1 if none
 * (GetInboundACL / GetOutboundACL, :215-225). */
int cls_if_acls(cls_engine* e, uint32_t if_id, int32_t* in_table, int32_t* out_table);

/* ---- batched connection verdicts (testConnection, :394-471) -------------
 * For each connection i: SYN through src_if inbound then dst_if outbound
 * with (src->dst, dport); SYN-ACK through dst_if inbound then src_if outbound
 * with (dst->src, sport); REFLECT marks sides reflected exactly as the
 * reference does.  Interface->ACL bindings are snapshotted at the call.
 * Addresses: CLS_AF_V4 (src4/dst4) or CLS_AF_V16 (src16/dst16, 16-byte
 * aligned on the device; IPv4-mapped = IPv4, as Go's To4) -- Connection*
 * takes any net.IP (:243-390).  A device batch's interface id outside the
 * engine's ids gives CLS_CONN_FAILURE for that connection (a host batch is
 * rejected with CLS_E_INVAL).  At most 2^30 connections per call.
 * Large ACLs: in batches >= 65536, an ACL with a compiled classifier image
 * whose linear work would be large (host batch: connections touching it x
 * its rules >= 2048 x batch, touches estimated from a hashed sample of <= 64
 * Ki connections -- a heuristic, verdicts do not depend on it; device batch:
 * >= 2048 rules) is evaluated by the classifier kernel for both tuples of
 * every connection before the connection kernel runs; the others by a linear
 * scan of compact rules, staged in LDS when they fit.  CLS_F_CONN_CLS: every
 * imaged ACL (>= 64 rules) at any batch size; CLS_F_FORCE_LINEAR: none.
 * CLS_F_COUNT: for every evalACL call the batch makes on a non-nil ACL (only
 * the calls testConnection makes, in its order), the table's connection
 * counter of the terminating rule (R: default DENY) is incremented.
 */
typedef struct cls_conn_soa {
    cls_pkt_soa pkt;           /* src/dst/sport/dport/proto of the SYN */
    const uint32_t* src_if;    /* interface ids (cls_if_id) */
    const uint32_t* dst_if;
} cls_conn_soa;

/* The connection path's floor: the average time of a kernel that reads the
 * 22 bytes of every IPv4 connection of a device batch (src, dst, src_if,
 * dst_if, sport, dport, proto) and writes one byte, without evaluating
 * anything, over `reps` launches (whole groups of 4 connections; 16-B aligned
 * src / dst / src_if / dst_if, 8-B ports, 4-B proto and out). */
int cls_stream_floor_conn(cls_engine* e, const cls_conn_soa* conns, uint64_t n, uint8_t* out,
                          uint32_t reps, float* ms, void* stream);
int cls_connect_batch(cls_engine* e, const cls_conn_soa* conns, uint64_t n,
                      uint8_t* conn_verdict_out, uint32_t flags, void* stream);

/* The trace twin of cls_connect_batch: besides the ConnectionAction (as
 * there; conn_verdict_out may be NULL), the rule at which every evalACL call
 * of testConnection ended -- what the reference logs per call (:651-654).
 * rule_out[4 i + k] is the k-th call of connection i in testConnection's
 * order: k = 0 SYN through src_if's inbound ACL, 1 SYN through dst_if's
 * outbound, 2 SYN-ACK through dst_if's inbound, 3 SYN-ACK through src_if's
 * outbound.  Each entry is the rule's index in that ACL's table, R for the
 * default DENY (:667), or -1 when testConnection does not make the call or
 * makes it on a nil ACL.  The tables are those of the bindings snapshotted at
 * the call: cls_if_acls(src_if / dst_if) names them (in_table for k = 0 and
 * 2, out_table for k = 1 and 3).  A device batch's connection with an unknown
 * interface id gives CLS_CONN_FAILURE and four -1 (a host batch is rejected
 * with CLS_E_INVAL).  Flags: CLS_F_DEVICE (device arrays, rule_out 16-byte
 * aligned, stream-ordered like cls_connect_batch; a host batch returns with
 * the results), CLS_F_CONN_CLS and CLS_F_FORCE_LINEAR as there; CLS_F_COUNT
 * is CLS_E_INVAL: the trace touches no counters.  At most 2^30 connections
 * per call. */
int cls_connect_rules(cls_engine* e, const cls_conn_soa* conns, uint64_t n,
                      uint8_t* conn_verdict_out, int32_t* rule_out,
                      uint32_t flags, void* stream);

/* Per-(ACL, rule) hit counters of the connection path: counters_out[k]
 * (k < R) = evalACL calls of cls_connect_batch (CLS_F_COUNT) on this table that
 * terminated at rule k, counters_out[R] = calls that fell through to the
 * default DENY (:667); summed over calls since the table was put or last
 * reset (reset != 0 clears them after the read).  Waits for pending device
 * work.  The reference has no counters. */
int cls_conn_counters(cls_engine* e, uint32_t table_id, uint64_t* counters_out, uint32_t reset);

/* ---- reachability matrix (ConnectionPodToPod looped over pods and ports,
 * aclengine_mock.go:243-300) ----------------------------------------------
 * Who reaches whom, on which probe: testConnection over every (probe,
 * source, destination) cell of N endpoints x P probes in one call, evaluated
 * on the device from the endpoint and probe lists -- the P x N x N rows a
 * connection batch would need are never built by the caller.  Cell (p, s, d),
 * at index (p N + s) N + d, is exactly testConnection(if_id[s], addr[s],
 * if_id[d], addr[d], proto[p], sport[p], dport[p]); the diagonal and the
 * pairs that share an interface are included (the same-interface REFLECT
 * short-cuts, :412-421, apply as in a batch).  The bindings are snapshotted
 * once for the whole call.  The arrays of `spec` are host memory, copied
 * before the call returns.  Outputs, each optional (not all three NULL):
 *   verdict_out [P][N][N]  ConnectionAction per cell (NULL: CLS_F_NO_VERDICT)
 *   hist_out    [P][4]     cells per ConnectionAction
 *   allow_out   [P][N]     per (probe, source) the destinations with CLS_CONN_ALLOW
 * hist_out and allow_out are overwritten, not accumulated.  Flags:
 * CLS_F_DEVICE -- the outputs are device memory on the engine's GPU
 * (verdict_out 16-byte, hist_out 8-byte, allow_out 4-byte aligned) and the
 * call only enqueues on `stream`, ordered like a device connection batch;
 * without it they are host arrays and the call returns with the results.
 * CLS_F_NO_VERDICT: verdict_out may be NULL.  CLS_F_COUNT, CLS_F_CONN_CLS,
 * CLS_F_FORCE_LINEAR: as cls_connect_batch (with CLS_F_COUNT the connection
 * counters afterwards show which rules no endpoint pair can hit).  The
 * matrix is evaluated in tiles of at most `reach_tile` connections
 * (cls_engine_set_option), each a device connection batch over engine-owned
 * scratch.  CLS_E_INVAL, before any device work: N or P zero, a bad af, a
 * NULL array, no output, verdict_out NULL without CLS_F_NO_VERDICT, a
 * misaligned device output, an unknown interface id, P N^2 > 2^36.  On a
 * multi-device engine the call runs on the first device. */
typedef struct cls_reach_spec {
    uint32_t af;                 /* CLS_AF_V4: addr4; CLS_AF_V16: addr16 (IPv4-mapped = IPv4) */
    uint32_t n_endpoints;        /* N >= 1 */
    const uint32_t* if_id;       /* N interface ids (cls_if_id) */
    const uint32_t* addr4;       /* N host-order IPv4 */
    const uint8_t* addr16;       /* N x 16 network-order bytes */
    uint32_t n_probes;           /* P >= 1 */
    const uint8_t* proto;        /* P ProtocolType */
    const uint16_t* sport;       /* P */
    const uint16_t* dport;       /* P */
} cls_reach_spec;
int cls_reach_matrix(cls_engine* e, const cls_reach_spec* spec, uint8_t* verdict_out,
                     uint64_t* hist_out, uint32_t* allow_out, uint32_t flags, void* stream);

/* ---- reachability diff: the changed cells of a matrix against a baseline --
 * "What connectivity did this commit change?"  Evaluates the matrix of `spec`
 * exactly as cls_reach_matrix does (the bindings snapshotted once) and
 * compares it on the device with `base`, a [P][N][N] matrix of an earlier
 * call: cell i is changed when base[i] != new[i] (the whole byte).  Neither
 * matrix has to cross PCIe.  Outputs (cls_reach_diff_out), each optional:
 *   verdict_out [P][N][N]  the new matrix; NULL, or == base exactly: the
 *                          baseline is refreshed in place (a tile's verdicts
 *                          reach it only after its base bytes were compared)
 *   hist_out, allow_out    of the new matrix, as cls_reach_matrix
 *   changes, cap           the first min(*n_changes, cap) changed cells in
 *                          ascending cell index (p N + s) N + d, whatever
 *                          reach_tile, the evaluator and the scheduling of
 *                          workgroups; records at and past that count are
 *                          not written
 *   n_changes   1 word     all changed cells, also those beyond cap
 *   trans_out   [P][4][4]  cells of probe p per (base & 3, new), unchanged
 *                          ones included: row sums are the old histogram,
 *                          column sums equal hist_out
 *   changed_out [P][N]     changed cells per (probe, source); overwritten
 * At least one of changes, n_changes, trans_out, changed_out must be given
 * (without them the request is cls_reach_matrix); changes needs n_changes
 * and cap >= 1.  Flags: CLS_F_DEVICE -- base and every output are device
 * memory (base, verdict_out, changes 16-byte; hist_out, n_changes, trans_out
 * 8-byte; allow_out, changed_out 4-byte aligned), the call only enqueues on
 * `stream`, ordered like a device connection batch.  Without it all are host
 * arrays and the call returns with the results: base goes up tile by tile,
 * the records come back through an engine-owned buffer, and no caller
 * pointer is kept.  CLS_F_COUNT, CLS_F_CONN_CLS, CLS_F_FORCE_LINEAR: as
 * cls_reach_matrix.  CLS_E_INVAL, before any device work and with the
 * outputs untouched: everything cls_reach_matrix refuses of `spec`, `out` or
 * `base` NULL, none of the four diff outputs, changes without n_changes or
 * with cap 0, a misaligned device pointer, verdict_out overlapping base
 * without being equal to it. */
typedef struct cls_reach_change {
    uint32_t probe, src, dst;    /* cell (p, s, d) */
    uint8_t was, now;            /* the base byte (verbatim), the new ConnectionAction */
    uint16_t zero;
} cls_reach_change;              /* 16 bytes, written with one 16-byte store */

typedef struct cls_reach_diff_out {
    uint8_t* verdict_out;
    uint64_t* hist_out;
    uint32_t* allow_out;
    cls_reach_change* changes;
    uint64_t cap;
    uint64_t* n_changes;
    uint64_t* trans_out;
    uint32_t* changed_out;
} cls_reach_diff_out;
int cls_reach_diff(cls_engine* e, const cls_reach_spec* spec, const uint8_t* base,
                   const cls_reach_diff_out* out, uint32_t flags, void* stream);

/* ---- reachability port sweep: per-pair port ranges over all 65,536 ports --
 * "On which destination ports does s reach d?"  Cell (s, d, port) is
 * testConnection(if_id[s], addr[s], if_id[d], addr[d], proto, sport, port)
 * for every port 0..65535, with `spec` as in cls_reach_matrix but exactly one
 * probe (proto[0], sport[0]; dport is ignored and may be NULL); the bindings
 * are snapshotted once, the diagonal and same-interface pairs included.
 * evalACL (:527-643) sees the destination port only in comparisons with
 * uint16(LowerPort) / uint16(UpperPort) of TCP / UDP rules, so a pair's
 * ConnectionAction is constant on every port class: the elementary intervals
 * whose starts are {0}, lo16 and hi16 + 1 of the swept protocol's rules over
 * the ACLs bound to the endpoints' interfaces (K classes).  The engine
 * evaluates one representative per class -- K N^2 connections, rows
 * (s N + d) K + k in tiles of whole pairs -- and compresses them on the
 * device.  Outputs (cls_reach_ports_out), each optional:
 *   ranges, cap   the first min(*n_ranges, cap) maximal ranges (adjacent
 *                 classes of equal action merged) in ascending (src, dst,
 *                 port_lo) order; the ranges of one pair tile [0, 65535].
 *                 Canonical: they depend on the verdicts alone, not on the
 *                 classes, reach_tile, the evaluator or the scheduling.
 *                 Records at and past that count are not written
 *   n_ranges      1 word: all ranges, also those beyond cap
 *   runs_out        [N][N]  ranges of the pair
 *   allow_ports_out [N][N]  dports with CLS_CONN_ALLOW, 0 .. 65536
 *   hist_out        [4]     (pair, dport) cells per ConnectionAction (sum 65536 N^2)
 *   n_classes     HOST word, also with CLS_F_DEVICE: K, written before the
 *                 call returns
 * At least one of ranges, n_ranges, runs_out, allow_ports_out, hist_out must
 * be given; ranges needs n_ranges and cap >= 1.  Any protocol is accepted:
 * for anything but TCP / UDP no rule tests the port, K = 1 and every pair has
 * the one range 0..65535.  Flags: CLS_F_DEVICE -- every output but n_classes
 * is device memory (ranges 16-byte, n_ranges and hist_out 8-byte, runs_out
 * and allow_ports_out 4-byte aligned) and the call only enqueues on `stream`,
 * ordered like a device connection batch; without it they are host arrays,
 * filled through engine-owned buffers (no caller pointer is kept).
 * CLS_F_CONN_CLS, CLS_F_FORCE_LINEAR: as cls_reach_matrix.  CLS_E_INVAL,
 * before any device work and with the outputs untouched: everything
 * cls_reach_matrix refuses of `spec` (but the NULL dport), n_probes != 1,
 * `out` NULL, no output, ranges without n_ranges or with cap 0, a misaligned
 * device pointer, CLS_F_COUNT or CLS_F_NO_VERDICT (representatives are
 * evaluated: connection counters would mean nothing), K N^2 > 2^36 (K and N
 * in cls_last_error).  On a multi-device engine the call runs on the first
 * device. */
typedef struct cls_port_range {  /* 16 bytes */
    uint32_t src, dst;           /* endpoint indices */
    uint16_t port_lo, port_hi;   /* inclusive */
    uint8_t action;              /* ConnectionAction for every dport in [port_lo, port_hi] */
    uint8_t zero[3];
} cls_port_range;

typedef struct cls_reach_ports_out {
    cls_port_range* ranges;
    uint64_t cap;
    uint64_t* n_ranges;
    uint32_t* runs_out;
    uint32_t* allow_ports_out;
    uint64_t* hist_out;
    uint32_t* n_classes;
} cls_reach_ports_out;
int cls_reach_ports(cls_engine* e, const cls_reach_spec* spec, const cls_reach_ports_out* out,
                    uint32_t flags, void* stream);
/* The class starts of one rule list for `proto` (no device needed): ascending,
 * lo_out[0] == 0, each in {0}, lo16 or hi16 + 1 <= 65535 of the rules that
 * carry a destination range for `proto` (the u16 values evalACL compares
 * with); K = 1 for anything but TCP / UDP.  *n = K; with cap < K only *n is
 * set.  cls_reach_ports uses the sorted union over the bound ACLs. */
int cls_port_classes(const cls_rule* rules, uint32_t n_rules, uint32_t proto,
                     uint16_t* lo_out, uint32_t cap, uint32_t* n);

/* ---- reachability hops: multi-hop closure and blast radius of the matrix ---
 * "If endpoint s is compromised, what can it reach in any number of hops, and
 * how many hops away is each endpoint?"  The graph: the N endpoints, with an
 * edge s -> d (s != d) iff the cell byte of (p, s, d) equals CLS_CONN_ALLOW
 * for at least one probe p (the union over probes; a per-probe answer is a
 * call with one probe).  Any other byte is no edge, and the diagonal is
 * ignored.  hops[s][d] is the length of a shortest path if it is at most H,
 * else CLS_HOPS_NONE; hops[s][s] == 0.  H is max_hops, 0 meaning 254.  Every
 * output (cls_reach_hops_out), each optional but not all NULL, is a function
 * of hops alone, so independent of reach_tile, the evaluator, hops_rows and
 * the scheduling:
 *   hops_out    [N][N]  the hop counts
 *   reach_out   [N]     per source the destinations d != s with hops <= H
 *                       (its blast radius)
 *   exposed_out [N]     per destination the sources s != d that reach it
 *   level_out   [256]   pairs (s, d) per hops value; [0] == N, [255] the
 *                       unreached
 *   closure_out [N][W]  W = (N + 63) / 64: bit (d & 63) of word d >> 6 of row
 *                       s is set iff hops[s][d] != CLS_HOPS_NONE; the padding
 *                       bits are zero
 * matrix == NULL: the matrix of `spec` is evaluated exactly as
 * cls_reach_matrix does (bindings snapshotted once, the same tiles,
 * CLS_F_CONN_CLS / CLS_F_FORCE_LINEAR / CLS_F_COUNT as there: the whole matrix
 * is evaluated), but its P N^2 verdict bytes never leave the tile scratch:
 * each tile's ALLOW cells are folded into an engine-owned bitmap of N W
 * words.  matrix != NULL: a [P][N][N] matrix of an earlier call -- device
 * memory, 16-byte aligned, with CLS_F_DEVICE, else host memory, which goes
 * up tile by tile through engine-owned scratch (no caller pointer is kept) --
 * is folded instead and no ACL is evaluated: only n_endpoints and n_probes of
 * `spec` are read (the arrays may be NULL), and the evaluator flags and
 * CLS_F_COUNT are refused.  Flags: CLS_F_DEVICE -- the outputs are device
 * memory (hops_out 16-byte, level_out and closure_out 8-byte, reach_out and
 * exposed_out 4-byte aligned) and the call only enqueues on `stream`, ordered
 * like a device connection batch; without it they are host arrays, filled
 * through engine-owned buffers.  CLS_E_INVAL, before any device work and with
 * the outputs untouched: everything cls_reach_matrix refuses of `spec` (with
 * a matrix only N or P zero and the cell bound), `out` NULL, no output,
 * CLS_F_NO_VERDICT, a misaligned device pointer, max_hops > 254, N > 32,768
 * (N in cls_last_error; a bit row is then at most 4 KiB, so that a
 * workgroup's rows fit LDS, and hops_out at most 1 GiB).  The hops_rows
 * option (cls_engine_set_option): the source rows a workgroup of the search
 * owns, 4, 8 or 16 (0, the default: 4).  On a multi-device engine the call
 * runs on the first device. */
#define CLS_HOPS_NONE 255u   /* not reached within max_hops */

typedef struct cls_reach_hops_out {
    uint8_t* hops_out;
    uint32_t* reach_out;
    uint32_t* exposed_out;
    uint64_t* level_out;
    uint64_t* closure_out;
} cls_reach_hops_out;
int cls_reach_hops(cls_engine* e, const cls_reach_spec* spec, const uint8_t* matrix,
                   uint32_t max_hops, const cls_reach_hops_out* out, uint32_t flags, void* stream);

/* ---- reachability classes: equivalent endpoints and their quotient matrix --
 * The summary of a [P][N][N] matrix: the groups of endpoints the policy
 * cannot tell apart, and the verdict between groups.  Cells are whole bytes.
 * Endpoints s and t are equivalent iff exchanging s and t leaves the matrix
 * unchanged; for every probe p:
 *   M[p,s,d] == M[p,t,d] and M[p,d,s] == M[p,d,t] for all d not in {s, t};
 *   M[p,s,t] == M[p,t,s];
 *   M[p,s,s] == M[p,t,t].
 * Transpositions that are automorphisms generate a group, so this is an
 * equivalence relation.  The diagonal (self connection, the same-interface
 * REFLECT short-cut) may differ from the off-diagonal.  Within a class all
 * diagonal cells are equal and all off-diagonal cells are equal; between two
 * classes all cells are equal.  So the matrix is exactly reconstructible from
 *   class[N]       the class of each endpoint
 *   self[P][C]     the diagonal value of each class
 *   quot[P][C][C]  the value between classes; quot[p][A][A] is the intra-class
 *                  off-diagonal value, or CLS_CLASS_NONE for a one-member class
 * Classes are numbered by ascending smallest member: class[0] == 0, and
 * rep[c], the first s with class[s] == c, is strictly ascending.  The result
 * is the coarsest such partition and depends on the matrix alone: not on
 * reach_tile, the evaluator, scheduling or hashing.
 * matrix == NULL: the matrix of `spec` is evaluated exactly as
 * cls_reach_matrix does (the same tiles, bindings snapshotted once for the
 * whole call, CLS_F_CONN_CLS / CLS_F_FORCE_LINEAR as there).  matrix != NULL:
 * a matrix of an earlier call, host memory or, with CLS_F_DEVICE, device
 * memory: only n_endpoints and n_probes of `spec` are read and the evaluator
 * flags are refused (cls_reach_hops).
 * How: a fold pass streams every tile and adds, per probe, 64-bit keyed sums
 * (wrapping, so independent of order) of each row and column off the
 * diagonal; the host groups endpoints whose sums and diagonals agree (in
 * every round so far); a verify pass streams the matrix again -- evaluated again, or read
 * from verdict_out / matrix in device memory -- and checks every cell against
 * the one value of its (probe, class, class) entry.  Only a collision of keys
 * can fail it, and then another round with new keys refines the partition, so
 * the result is exact whatever the keys.  *rounds is the number of rounds
 * taken: 1 at the full key width.  The classes_key_bits option
 * (cls_engine_set_option, 0 .. 64, default 64; diagnostics) keeps only the low
 * bits of the sums in the keys to force collisions; after 16 rounds the call
 * returns CLS_E_INVAL ("did not converge"), which only that option reaches.
 * Scratch that cannot be allocated: CLS_E_NOMEM.
 * Outputs (cls_reach_classes_out): at least one of class_out and n_classes;
 * the per-class outputs rep_out, size_out, self_out, quot_out hold up to
 * class_cap classes and are written only when C <= class_cap -- otherwise they
 * stay untouched, class_out and *n_classes are still written and the call
 * returns CLS_OK: the caller retries with room.  verdict_out, optional: the
 * evaluated matrix (with a matrix given: a copy of it).  n_classes, rounds and
 * sums_out (diagnostics: [P][N][2] row and column sums of the last round) are
 * HOST memory also with CLS_F_DEVICE, under which the matrix and every other
 * output are device memory (verdict_out and matrix 16-byte, the u32 arrays
 * 4-byte aligned) and the device work runs on `stream`.
 * Unlike the other reach calls this one RETURNS ONLY WHEN THE RESULT IS
 * COMPLETE, also with CLS_F_DEVICE: the class count and the verify pass's
 * result decide what is enqueued next.
 * CLS_E_INVAL, before any device work and with the outputs untouched:
 * everything cls_reach_hops refuses for the same form, CLS_F_COUNT,
 * CLS_F_NO_VERDICT, N > 32,768, neither class_out nor n_classes, per-class
 * outputs with class_cap == 0, a misaligned device pointer.  On a
 * multi-device engine the call runs on the first device. */
#define CLS_CLASS_NONE 255u  /* quot[p][A][A] of a one-member class */

typedef struct cls_reach_classes_out {
    uint32_t* class_out;    /* [N] class of each endpoint */
    uint32_t* n_classes;    /* HOST word, also with CLS_F_DEVICE: C */
    uint64_t class_cap;     /* the per-class outputs hold up to class_cap classes */
    uint32_t* rep_out;      /* [C] smallest member */
    uint32_t* size_out;     /* [C] members */
    uint8_t* self_out;      /* [P][C] */
    uint8_t* quot_out;      /* [P][C][C], dense in C */
    uint8_t* verdict_out;   /* [P][N][N] optional: the evaluated matrix */
    uint32_t* rounds;       /* HOST word, diagnostics: rounds taken */
    uint64_t* sums_out;     /* HOST, diagnostics: [P][N][2] row and column sums of the last round */
} cls_reach_classes_out;
int cls_reach_classes(cls_engine* e, const cls_reach_spec* spec, const uint8_t* matrix,
                      const cls_reach_classes_out* out, uint32_t flags, void* stream);
/* The device-free twin: the same pipeline on the host over a host matrix,
 * with the same keys, seeds, grouping and round loop, so that its sums_out
 * and rounds equal the device call's bit for bit.  key_bits: 0 .. 64 (the
 * classes_key_bits option; 64 for the exact single round).  Every pointer is
 * host memory.  CLS_E_INVAL: matrix NULL, N or P zero, above 2^36 cells,
 * N > 32,768, key_bits > 64, the outputs' refusals above, or no convergence
 * within 16 rounds; the outputs are then untouched. */
int cls_reach_classes_host(const uint8_t* matrix, uint32_t n_endpoints, uint32_t n_probes, uint32_t key_bits,
                           const cls_reach_classes_out* out);

/* ---- reachability external sweep: per-pod address ranges over all of IPv4 --
 * "Which remote addresses can this pod talk to, and which can reach it?" --
 * ConnectionPodToInternet / ConnectionInternetToPod (aclengine_mock.go:303-390)
 * for every IPv4 address at once.  `spec` is as for cls_reach_matrix: N
 * endpoints, P probes (at most 65,536: a record's probe is 16 bits); ext_if
 * is the id (cls_if_id) of the node's output interface, which the caller
 * resolves as ConnectionPodToInternet does.  `dirs` is a set of CLS_EXT_*
 * bits; D is their number and the directions are indexed in ascending order
 * of their bit.  For every IPv4 address a
 *   egress  cell (p, s, a): testConnection(if_id[s], addr[s], ext_if, a,
 *                                          proto[p], sport[p], dport[p])
 *   ingress cell (p, s, a): testConnection(ext_if, a, if_id[s], addr[s], ...)
 * the pods' own range included (the reference does not exclude it); in the
 * 16-byte layout a is the IPv4-mapped ::ffff:a and endpoints may be native
 * IPv6.  The bindings are snapshotted once; the same-interface REFLECT
 * short-cuts apply where if_id[s] == ext_if.
 * evalACL (:499-524) sees the remote address only in IPNet.Contains tests of
 * the rules' parsed networks, and a parsed network holds no IPv4 address or
 * one aligned interval of them, so a cell's ConnectionAction is constant on
 * every address class: the elementary intervals whose starts are {0}, lo and
 * hi + 1 <= 2^32 - 1 of every source or destination network of effective
 * family 4 (strings that fail to parse and family-16 networks contribute
 * nothing) over the ACLs bound, inbound or outbound, to the endpoints'
 * interfaces and to ext_if (K classes).  The engine evaluates one
 * representative per class -- D P N K connections; a line is one (dir, probe,
 * endpoint), numbered (d P + p) N + s, rows line K + k in tiles of
 * max(1, reach_tile / K) whole lines -- and compresses them on the device.
 * Outputs (cls_reach_ext_out), each optional:
 *   ranges, cap   the first min(*n_ranges, cap) maximal ranges (adjacent
 *                 classes of equal action merged) in ascending (dir, probe,
 *                 src, addr_lo) order; the ranges of one line tile
 *                 [0, 0xFFFFFFFF].  Canonical: they depend on the verdicts
 *                 alone, not on the classes, reach_tile, the evaluator or the
 *                 scheduling.  Records at and past that count are not written
 *   n_ranges      1 word: all ranges, also those beyond cap
 *   runs_out        [D][P][N]  ranges of the line
 *   allow_addrs_out [D][P][N]  addresses with CLS_CONN_ALLOW, 0 .. 2^32
 *   hist_out        [D][P][4]  addresses per ConnectionAction (each row of 4
 *                              sums to 2^32 N)
 *   n_classes     HOST word, also with CLS_F_DEVICE: K, written before the
 *                 call returns
 * At least one of ranges, n_ranges, runs_out, allow_addrs_out, hist_out must
 * be given; ranges needs n_ranges and cap >= 1.  Flags: CLS_F_DEVICE -- every
 * output but n_classes is device memory (ranges 16-byte, n_ranges,
 * allow_addrs_out and hist_out 8-byte, runs_out 4-byte aligned) and the call
 * only enqueues on `stream`, ordered like a device connection batch; without
 * it they are host arrays, filled through engine-owned buffers (no caller
 * pointer is kept).  CLS_F_CONN_CLS, CLS_F_FORCE_LINEAR: as cls_reach_matrix.
 * CLS_E_INVAL, before any device work and with the outputs untouched:
 * everything cls_reach_matrix refuses of `spec`, more than 65,536 probes,
 * dirs zero or with other bits, an unknown ext_if, `out` NULL, no output,
 * ranges without n_ranges or with cap 0, a misaligned device pointer,
 * CLS_F_COUNT or CLS_F_NO_VERDICT (representatives are evaluated: connection
 * counters would mean nothing), D P N K > 2^36 (K and N in cls_last_error),
 * K > 2^30.  On a multi-device engine the call runs on the first device. */
enum { CLS_EXT_EGRESS = 1u, CLS_EXT_INGRESS = 2u };

typedef struct cls_addr_range {  /* 16 bytes */
    uint32_t src;                /* endpoint index */
    uint16_t probe;
    uint8_t dir;                 /* 0 egress (pod -> address), 1 ingress (address -> pod) */
    uint8_t action;              /* ConnectionAction for every address in [addr_lo, addr_hi] */
    uint32_t addr_lo, addr_hi;   /* host-order IPv4, inclusive */
} cls_addr_range;

typedef struct cls_reach_ext_out {
    cls_addr_range* ranges;
    uint64_t cap;
    uint64_t* n_ranges;
    uint32_t* runs_out;
    uint64_t* allow_addrs_out;
    uint64_t* hist_out;
    uint32_t* n_classes;
} cls_reach_ext_out;
int cls_reach_external(cls_engine* e, const cls_reach_spec* spec, uint32_t ext_if, uint32_t dirs,
                       const cls_reach_ext_out* out, uint32_t flags, void* stream);
/* The address class starts of one rule list (no device needed): ascending,
 * lo_out[0] == 0, each in {0}, lo or hi + 1 <= 2^32 - 1 of a source or
 * destination network whose effective family is 4 (a.b.c.d/n, or an IPv6
 * string whose masked address is IPv4-mapped).  *n = K; with cap < K only *n
 * is set.  cls_reach_external uses the sorted union over the bound ACLs. */
int cls_addr_classes(const cls_rule* rules, uint32_t n_rules, uint32_t* lo_out, uint32_t cap, uint32_t* n);

/* ---- rule coverage sweep: dead rules and a witness packet per rule ---------
 * "Which rules of this table can never be the matched rule, for any packet?
 * For the others, show me a packet that matches each one."  The space is every
 * IPv4 packet (src, dst, proto, dport): src and dst 0 .. 2^32 - 1, proto a
 * uint8, dport 0 .. 65535; with af CLS_AF_V16 the same packets go to the
 * 16-byte classifier as ::ffff:src / ::ffff:dst.  Native IPv6 packets are out
 * of scope: a rule that only IPv6 packets can reach is reported dead by this
 * IPv4 sweep.
 * evalACL (aclengine_mock.go:473-668) sees a packet in four ways only: the
 * source address in Contains tests of source networks, the destination address
 * in Contains tests of destination networks, the protocol through one switch,
 * the destination port in comparisons with the u16 range ends of that
 * protocol's section.  So the terminating rule is constant on every cell of
 *   Ks source classes: the elementary intervals whose starts are {0}, lo and
 *      hi + 1 <= 2^32 - 1 of every SOURCE network of effective family 4
 *      (cls_addr_classes' rules, per side: cls_cover_classes side 0);
 *   Kd destination classes: the same of the DESTINATION networks (side 1);
 *   T = Kt + Ku + 2 columns, in this order: the table's TCP port classes
 *      ascending (cls_port_classes), its UDP port classes, one ICMP column
 *      (port 0), one column for every other protocol value (representative:
 *      protocol 3, port 0).
 * Cell c = (s Kd + d) T + j; its representative is the lowest packet of each
 * class, so ascending c is ascending (src, dst, proto, dport) of the
 * representatives.  The engine evaluates the cells in tiles of cover_tile --
 * cells expanded on the device, the matched-rule trace of cls_classify_rules
 * unchanged, no counters touched -- and folds them there.
 * "Terminates at k" is the counters' definition, whatever the action: a
 * FAILURE at a rule counts for that rule; index R is the default DENY.
 * Outputs (cls_cover_out), each optional:
 *   live_out    [R+1] u8   1 iff some packet of the space terminates at rule k
 *   witness_out [R+1]      the least such packet in (src, dst, proto, dport)
 *                          order, protocol 3 standing for every value above
 *                          2; all zero for a dead rule.  Canonical: it depends
 *                          on the rule list's semantics alone, not on the
 *                          classes, cover_tile, the evaluator or the
 *                          scheduling (the least hitting packet is the low
 *                          corner of the lowest hitting cell)
 *   cells_out   [R+1] u64  the cells terminating at the rule: defined relative
 *                          to the classes above, a deterministic function of
 *                          the rule list; sums to Ks Kd T (every cell folded
 *                          exactly once)
 *   n_dead      1 word     rules k < R with live == 0
 *   n_cells     HOST word, also with CLS_F_DEVICE: Ks Kd T
 *   dims        HOST [4], also with CLS_F_DEVICE: Ks, Kd, Kt, Ku
 * At least one of live_out, witness_out, cells_out, n_dead must be given.
 * Flags: CLS_F_DEVICE -- those four are device memory (witness_out 16-byte,
 * cells_out 8-byte, n_dead 4-byte aligned) and the call only enqueues on
 * `stream`; without it they are host arrays filled through engine-owned
 * buffers.  CLS_F_FORCE_LINEAR -- the linear kernel evaluates; it is the IPv4
 * one in either layout (the sweep's 16-byte packets are IPv4-mapped, and the
 * 16-byte layout's linear form writes no rule).  CLS_E_INVAL, before any
 * device work and with every output untouched: af other than CLS_AF_V4 /
 * CLS_AF_V16, a CLS_AF_V16 sweep of a table without a 16-byte classifier (as
 * cls_classify_rules), `out` NULL or none of the four outputs, a misaligned
 * device pointer, any other flag, Ks Kd T > 2^40 (the three factors in
 * cls_last_error).  CLS_E_NOTFOUND: an unknown table.  The call takes the
 * engine's lock and the table as classify calls do and restores the caller's
 * device; on a multi-device engine it runs on the first device. */
typedef struct cls_cover_witness {   /* 16 bytes */
    uint32_t src, dst;               /* host-order IPv4 */
    uint16_t dport;
    uint8_t proto;                   /* 0, 1, 2, or 3 standing for every value > 2 */
    uint8_t live;                    /* 1: some packet terminates at this rule */
    uint32_t zero;
} cls_cover_witness;

typedef struct cls_cover_out {
    uint8_t* live_out;               /* [R+1]  index R: the default DENY */
    cls_cover_witness* witness_out;  /* [R+1] */
    uint64_t* cells_out;             /* [R+1]  cells terminating at the rule; sums to Ks Kd T */
    uint32_t* n_dead;                /* 1 word: rules k < R with live == 0 */
    uint64_t* n_cells;               /* HOST word, also with CLS_F_DEVICE: Ks Kd T */
    uint32_t* dims;                  /* HOST [4], optional: Ks, Kd, Kt, Ku */
} cls_cover_out;

int cls_table_cover(cls_engine* e, uint32_t table_id, uint32_t af, const cls_cover_out* out, uint32_t flags,
                    void* stream);
/* The class starts of one side of a rule list (no device needed; side 0 =
 * source networks, 1 = destination networks): ascending, lo_out[0] == 0, as
 * cls_addr_classes over that side alone.  *n = K; with cap < K only *n is
 * set.  CLS_E_INVAL: side above 1. */
int cls_cover_classes(const cls_rule* rules, uint32_t n_rules, uint32_t side, uint32_t* lo_out, uint32_t cap,
                      uint32_t* n);

/* ---- table diff: packets whose verdict differs between two rule lists -------
 * "Is table b semantically the same as table a?  If not, for exactly which
 * packets does the verdict change, and which rules are responsible?"  The
 * space, the cells and their order are cls_table_cover's: every IPv4 packet
 * (src, dst, proto, dport), with af CLS_AF_V16 the same packets as ::ffff:a in
 * the 16-byte layout; native IPv6 packets are out of scope.  Both tables'
 * verdicts are constant on every cell of the JOINT classes -- per side and per
 * protocol the sorted union of the two tables' class starts, which equals
 * cls_cover_classes / cls_port_classes over the two rule lists concatenated
 * (a's rules, then b's) -- so Ks, Kd, Kt, Ku, T = Kt + Ku + 2, the cell index
 * c = (s Kd + d) T + j and the columns are cover's over that list.  The engine
 * evaluates the cells in tiles of whole rows (max(1, cover_tile / T) rows of T
 * cells) under both tables with the matched-rule trace of cls_classify_rules,
 * unchanged, and compares on the device.
 * A cell differs iff the two ACLActions differ.  Equal verdicts through
 * different rules are no difference: rule indices of different tables are not
 * comparable.  table_a == table_b is allowed and yields none.
 * Records (cls_tdiff_rec): one per maximal run of consecutive differing cells
 * that lies within one (source class, destination class) row and one protocol
 * and whose cells have equal (was, now, rule_a, rule_b); in ascending cell
 * order.  src_hi, dst_hi and port_hi are the next class start minus one, or the
 * top of the range.  The first min(rec_cap, total) records are written; *n_rec
 * is the total either way.
 * Outputs (cls_tdiff_out), each optional:
 *   n_diff    1 u64        cells with was != now
 *   pairs_out [4][4] u64   cells per (was, now); sums to n_cells
 *   first_out 1            the least differing packet in (src, dst, proto,
 *                          dport) order; live 0 and zeros if there is none
 *   cells_a   [Ra+1] u64   differing cells terminating at rule k of a (Ra: the
 *                          default DENY)
 *   wit_a     [Ra+1]       the least differing packet terminating at rule k of
 *                          a; zeros where there is none
 *   cells_b, wit_b [Rb+1]  the same for b
 *   rec_out, rec_cap, n_rec  the records (rec_out needs n_rec; n_rec alone
 *                          counts them)
 *   n_cells   HOST word, also with CLS_F_DEVICE: Ks Kd T
 *   dims      HOST [4], also with CLS_F_DEVICE: the joint Ks, Kd, Kt, Ku
 * first_out, wit_a and wit_b depend on the two lists' semantics alone (the
 * least packet of a union of cells is the low corner of its lowest cell under
 * any valid refinement); the counts and the records are defined relative to
 * the joint classes and the rule structure, a deterministic function of the
 * two lists.  No output depends on cover_tile, the evaluator or the
 * scheduling.
 * Flags: CLS_F_DEVICE -- every pointer not marked HOST is device memory
 * (records and witnesses 16-byte, the u64 arrays 8-byte aligned) and the call
 * only enqueues on `stream`; CLS_F_FORCE_LINEAR -- as cls_table_cover.
 * CLS_E_INVAL, before any device work and with every output untouched: any
 * other flag, af other than CLS_AF_V4 / CLS_AF_V16, a CLS_AF_V16 diff where
 * either table has no 16-byte classifier (the message names the table), `out`
 * NULL, none of the outputs given, rec_out without n_rec, rec_cap > 0 with
 * rec_out NULL, a misaligned device pointer, Ks Kd T > 2^40 (the three factors
 * in cls_last_error).  CLS_E_NOTFOUND: an unknown table on either side.  The
 * call takes the engine's lock once and both tables as classify calls do and
 * restores the caller's device; on a multi-device engine it runs on the first
 * device. */
typedef struct cls_tdiff_rec {      /* 32 bytes */
    uint32_t src_lo, src_hi, dst_lo, dst_hi;  /* host-order IPv4, inclusive */
    uint16_t port_lo, port_hi;                /* inclusive; 0 .. 65535 for proto 2 and 3 (port not examined) */
    uint8_t proto;                            /* 0, 1, 2, or 3 standing for every value > 2 */
    uint8_t was, now;                         /* ACLAction (CLS_ACL_*) under table a / table b; was != now */
    uint8_t zero;
    uint32_t rule_a, rule_b;                  /* terminating rule in a / in b (Ra / Rb: the default DENY) */
} cls_tdiff_rec;

typedef struct cls_tdiff_out {
    uint64_t* n_diff;              /* 1 word: cells with was != now */
    uint64_t* pairs_out;           /* [4][4]: cells per (was, now); sums to n_cells */
    cls_cover_witness* first_out;  /* 1: the least differing packet; live 0 and zeros if none */
    uint64_t* cells_a;             /* [Ra+1]: differing cells terminating at rule k of a */
    cls_cover_witness* wit_a;      /* [Ra+1]: least differing packet terminating at rule k of a */
    uint64_t* cells_b;             /* [Rb+1] */
    cls_cover_witness* wit_b;      /* [Rb+1] */
    cls_tdiff_rec* rec_out;        /* up to rec_cap records, ascending */
    uint64_t rec_cap;
    uint64_t* n_rec;               /* 1 word: the total, also above rec_cap */
    uint64_t* n_cells;             /* HOST word, also with CLS_F_DEVICE */
    uint32_t* dims;                /* HOST [4]: joint Ks, Kd, Kt, Ku */
} cls_tdiff_out;

int cls_table_diff(cls_engine* e, uint32_t table_a, uint32_t table_b, uint32_t af,
                   const cls_tdiff_out* out, uint32_t flags, void* stream);

/* ---- rule necessity sweep: rules a table can lose without changing a verdict
 * "Which rules does this list actually need?"  A rule can be live (packets
 * terminate at it) and still be removable: every packet it takes gets the same
 * ACLAction from the rest of the list once the rule is gone.  The space, the
 * classes, the cell numbering c = (s Kd + d) T + j and the columns are
 * cls_table_cover's (Table classes of the one list): every IPv4 packet (src,
 * dst, proto, dport).  Native IPv6 packets are out of scope: a rule with an
 * IPv6 network takes no IPv4 packet and is reported dead by this sweep.
 * For a table of R rules and an optional set `skip` of rules treated as
 * deleted (a HOST bitmask of (R + 63) / 64 u64 words, bit r & 63 of word r >>
 * 6, copied before the call returns; NULL: none):
 *   first(c)   the lowest rule outside skip that terminates cell c; R: the
 *              default DENY
 *   second(c)  the next such rule above first(c); R if none
 *   act(k, c)  rule k's ACLAction for the cell's protocol (a FAILURE at the
 *              rule is an action of its own); CLS_ACL_DENY for k = R
 *   cell c CHANGES UNDER r iff first(c) == r and act(second(c), c) != act(r, c)
 * In the reduced form of the rules (evalACL, aclengine_mock.go:473-668) "rule k
 * terminates packet x" is (source class of x in k's source set) AND
 * (destination class in k's destination set) AND (column in k's column set), so
 * the set of ALL rules that would take a cell is the AND of three bit rows, one
 * bit per rule: its lowest set bit is first, the next one second.  This
 * evaluator is independent of the compiled classifiers, which encode first
 * matches only.
 * Per rule r (need_out): CLS_NEED_SKIPPED -- r is in skip; CLS_NEED_DEAD -- no
 * cell has first == r; CLS_NEED_REDUNDANT -- some cell has, and none changes
 * under r; CLS_NEED_NEEDED -- some cell changes under r.  need[r] != NEEDED
 * holds exactly when the list without r alone (and without skip) gives every
 * IPv4 packet the same ACLAction.  Redundant rules are not jointly removable
 * (two equal PERMITs: each is redundant given the other), so free_out[r] = 1
 * iff r is DEAD, or r is REDUNDANT and every cell with first == r has a second
 * that is NEEDED or the default: all free rules can be deleted together
 * without changing a verdict, and unless no rule is dead or redundant at least
 * one rule is free.
 * Outputs (cls_need_out), each optional; one of the first six must be given:
 *   need_out    [R] u8     CLS_NEED_*
 *   free_out    [R] u8
 *   first_out   [R+1] u64  the cells with first == k under skip; sums to Ks Kd
 *                          T; with no skip cls_table_cover's cells_out
 *   changed_out [R] u64    the cells that change under r (relative to the
 *                          classes, a deterministic function of the list)
 *   witness_out [R]        for a NEEDED rule the LEAST packet in (src, dst,
 *                          proto, dport) order that changes under r, `after`
 *                          the ACLAction it gets without r with bit 7 set as
 *                          the valid mark, `fall` the rule that then takes it
 *                          (R: the default); all zero for every other rule.
 *                          Canonical as cls_table_cover's witness: the low
 *                          corner of the lowest changing cell
 *   counts      [4] u32    rules per CLS_NEED_* value
 *   n_cells     HOST word, also with CLS_F_DEVICE: Ks Kd T
 *   dims        HOST [4], also with CLS_F_DEVICE: Ks, Kd, Kt, Ku
 * No output depends on cover_tile (the sweep goes in tiles of max(1,
 * cover_tile / T) whole (s, d) pairs), on the need_cols_lds option (the column
 * rows in LDS or read from global memory) or on the scheduling.
 * Flags: CLS_F_DEVICE only -- the first six outputs are device memory
 * (witness_out 16-byte, first_out and changed_out 8-byte, counts 4-byte
 * aligned) and the call only enqueues on `stream`.  CLS_E_INVAL, before any
 * device work and with every output untouched: `out` NULL or none of the six
 * outputs, any other flag, a misaligned device pointer, Ks Kd T > 2^40, bit
 * rows -- (Ks + Kd + T + 1) rows of (R + 63) / 64 u64 words -- above the
 * need_bitmap_mb option's MiB (default 1024; the numbers in cls_last_error).
 * CLS_E_NOTFOUND: an unknown table.  Lock, table lifetime and the caller's
 * device as cls_table_cover. */
enum { CLS_NEED_SKIPPED = 0, CLS_NEED_DEAD = 1, CLS_NEED_REDUNDANT = 2, CLS_NEED_NEEDED = 3 };

typedef struct cls_need_witness {    /* 16 bytes */
    uint32_t src, dst;               /* host-order IPv4 */
    uint16_t dport;
    uint8_t proto;                   /* 0, 1, 2, or 3 standing for every value > 2 */
    uint8_t after;                   /* 0x80 | the ACLAction without the rule; 0: the rule is not NEEDED */
    uint32_t fall;                   /* the rule that takes the packet then; R: the default DENY */
} cls_need_witness;

typedef struct cls_need_out {
    uint8_t* need_out;               /* [R] */
    uint8_t* free_out;               /* [R] */
    uint64_t* first_out;             /* [R+1] */
    uint64_t* changed_out;           /* [R] */
    cls_need_witness* witness_out;   /* [R] */
    uint32_t* counts;                /* [4] */
    uint64_t* n_cells;               /* HOST word, also with CLS_F_DEVICE */
    uint32_t* dims;                  /* HOST [4]: Ks, Kd, Kt, Ku */
} cls_need_out;

int cls_table_need(cls_engine* e, uint32_t table_id, const uint64_t* skip, const cls_need_out* out, uint32_t flags,
                   void* stream);
/* The same definition with no device: plain C++ over the same bit rows (the
 * CPU baseline; every pointer host memory).  CLS_E_INVAL: `out` NULL or none
 * of the six outputs, rules NULL with n_rules > 0, a rule with nil Matches,
 * Ks Kd T > 2^40. */
int cls_table_need_host(const cls_rule* rules, uint32_t n_rules, const uint64_t* skip, const cls_need_out* out);

/* ---- synthetic traffic (BASELINE.md / SURVEY 8(d) generator) -----------
 * Generates packets i in [first, first+n) of the counter-based splitmix64
 * stream directly into device memory (no PCIe).  Pools: pod IPs, rule
 * destination prefixes (addr, prefix length) and ports drawn from the table.
 */
typedef struct cls_traffic_spec {
    uint64_t seed;
    uint32_t pct_pod_src;      /* % of packets whose src is a pod IP (60) */
    uint32_t pct_rule_dst;     /* % whose dst lies in a rule dst prefix (50) */
    uint32_t pct_table_port;   /* % whose dport is one of the table ports (50) */
    uint32_t pct_icmp;         /* % ICMP (0 or 10); the rest split TCP/UDP evenly */
    const uint32_t* pod_ips; uint32_t n_pod_ips;
    const uint32_t* dst_addrs; const uint8_t* dst_lens; uint32_t n_dst;
    const uint16_t* ports; uint32_t n_ports;
} cls_traffic_spec;
int cls_gen_traffic_v4(cls_engine* e, const cls_traffic_spec* spec, uint64_t first,
                       uint64_t n, uint32_t* src4, uint32_t* dst4, uint16_t* sport,
                       uint16_t* dport, uint8_t* proto, void* stream);

/* The 16-byte stream (config 5, mixed families): pools of 16-byte network-
 * order addresses (IPv4 as IPv4-mapped), destination prefix lengths 0..128.
 * Packet i draws w_k = splitmix64(seed ^ ((8i + k) * golden)), k < 8, as the
 * IPv4 stream does for protocol, ports and the pool choices; an address not
 * drawn from a pool is IPv6 fd00::/64 + w_6 (src) or w_7 (dst) when bit 0 of
 * the choice word's high half is set, else IPv4-mapped ::ffff:(u32)w_1 (src)
 * or (u32)w_3 (dst); a pool prefix's host bits come from (w_3, w_7). */
typedef struct cls_traffic_spec16 {
    uint64_t seed;
    uint32_t pct_pod_src, pct_rule_dst, pct_table_port, pct_icmp;
    const uint8_t* pod_ips; uint32_t n_pod_ips;            /* n x 16 bytes */
    const uint8_t* dst_addrs; const uint8_t* dst_lens; uint32_t n_dst;
    const uint16_t* ports; uint32_t n_ports;
} cls_traffic_spec16;
int cls_gen_traffic_v16(cls_engine* e, const cls_traffic_spec16* spec, uint64_t first,
                        uint64_t n, uint8_t* src16, uint8_t* dst16, uint16_t* sport,
                        uint16_t* dport, uint8_t* proto, void* stream);

/* ---- engine-owned batches (SURVEY 8(b) ownership, 8(e) sharding) --------
 * A batch is device memory the engine owns, so a caller that must not let
 * the library keep its pointers (cgo) can still run the HBM-resident path:
 * upload once (or generate on the device), classify many times, download
 * what it needs.  Packets [0, n) shard contiguously over the engine's
 * devices (cls_shard_range): shard g = [g n / G, (g + 1) n / G) lives in
 * device g's HBM.  Fields are structure-of-arrays, each array 256-B aligned
 * per shard (the classify kernels' 16-B loads): addresses u32 (CLS_AF_V4)
 * or 16 bytes (CLS_AF_V16), ports u16, protocol and verdict u8, interface
 * ids u32 (CLS_BATCH_CONN).  With CLS_BATCH_MIRROR the batch also owns a
 * pinned host copy of every field (hipHostMalloc; cls_batch_mirror) that
 * the caller fills or reads in place: uploads and downloads with a NULL
 * host pointer move it at DMA speed.  Without it, upload / download go
 * through the engine's pinned staging buffers.
 * Work on a batch runs on its devices' engine streams; a call returns once
 * the work is enqueued unless it returns host data (counters_out,
 * downloads, cls_batch_counters, cls_batch_wait). */
typedef struct cls_batch cls_batch;
enum {
    CLS_BF_SRC = 0, CLS_BF_DST = 1, CLS_BF_SPORT = 2, CLS_BF_DPORT = 3, CLS_BF_PROTO = 4,
    CLS_BF_VERDICT = 5,        /* cls_classify_batch: ACLAction; cls_batch_connect: ConnectionAction */
    CLS_BF_SRC_IF = 6, CLS_BF_DST_IF = 7,   /* CLS_BATCH_CONN only */
    CLS_BF_COUNT = 8
};
enum {
    CLS_BATCH_CONN = 1u << 0,    /* also interface ids (connection batches) */
    CLS_BATCH_MIRROR = 1u << 1   /* a pinned host mirror of every field */
};
/* Shard g of n packets over G devices: [g n / G, (g + 1) n / G). */
int cls_shard_range(uint64_t n, uint32_t n_shards, uint32_t shard, uint64_t* first, uint64_t* count);
int cls_batch_create(cls_engine* e, uint32_t af, uint64_t n, uint32_t flags, cls_batch** out);
void cls_batch_destroy(cls_batch* b);
int cls_batch_shards(const cls_batch* b, uint32_t* n_shards);
int cls_batch_shard(const cls_batch* b, uint32_t shard, int* device, uint64_t* first, uint64_t* n);
/* Device address of a field's array in shard `shard` (for a caller's own
 * kernels, e.g. a capture path writing packets in place). */
int cls_batch_field(cls_batch* b, uint32_t shard, uint32_t field, void** dev_ptr);
/* Host address of a field's pinned mirror (whole batch, packet order). */
int cls_batch_mirror(cls_batch* b, uint32_t field, void** host_ptr);
/* Packets [first, first + n) of one field from `src` (NULL: the mirror). */
int cls_batch_upload(cls_batch* b, uint32_t field, uint64_t first, uint64_t n, const void* src);
/* ... to `dst` (NULL: the mirror).  Waits for the batch's work. */
int cls_batch_download(cls_batch* b, uint32_t field, uint64_t first, uint64_t n, void* dst);
/* The synthetic stream into the batch on the devices: packet i of the batch
 * is stream packet stream_first + i (the same stream as cls_gen_traffic_*). */
int cls_batch_gen_traffic_v4(cls_batch* b, const cls_traffic_spec* spec, uint64_t stream_first);
int cls_batch_gen_traffic_v16(cls_batch* b, const cls_traffic_spec16* spec, uint64_t stream_first);
/* evalACL over every packet of the batch (verdicts into CLS_BF_VERDICT) with
 * the table's hit counters (as cls_classify) summed over the shards: by the
 * engine's RCCL communicator when it has one (an all-reduce over the
 * devices -- and over the processes of cls_comm_init -- on a side stream, so
 * it overlaps the next call's classify; two counter buffers alternate), else
 * on the host when read.  counters_out (host, R + 1): wait and write them
 * (CLS_F_ACCUMULATE: add); NULL: only enqueue (cls_batch_counters reads the
 * last call's).  Flags: CLS_F_NO_VERDICT, CLS_F_FORCE_LINEAR, CLS_F_TIMING
 * (each device's classify kernel is timed on that device's engine:
 * cls_kernel_times of cls_device_engine), CLS_F_ACCUMULATE. */
int cls_classify_batch(cls_engine* e, uint32_t table_id, cls_batch* b, uint64_t* counters_out, uint32_t flags);
/* Counters of the batch's last cls_classify_batch (n_out >= R + 1 of that
 * table); waits for them. */
int cls_batch_counters(cls_batch* b, uint64_t* out, uint32_t n_out);
/* testConnection over a CLS_BATCH_CONN batch (as cls_connect_batch with
 * device memory; ConnectionAction into CLS_BF_VERDICT), every device its
 * shard; CLS_F_COUNT counts into each device's copy of the tables'
 * connection counters (cls_conn_counters sums them).  Returns once the work
 * is enqueued on every device's engine stream: cls_batch_wait,
 * cls_batch_download and cls_conn_counters order behind it. */
int cls_batch_connect(cls_engine* e, cls_batch* b, uint32_t flags);
/* Wait for every device's work on the batch. */
int cls_batch_wait(cls_batch* b);

/* ---- the hit-counter all-reduce over processes (RCCL) --------------------
 * One process per GPU (or per group of GPUs): process 0 makes an id
 * (cls_comm_unique_id), every process receives it out of band and calls
 * cls_comm_init with the same n_procs; device g of process p is rank
 * p * G + g of n_procs * G (every process's engine has G devices).  From
 * then on cls_classify_batch all-reduces its counters over all ranks.
 * n_procs = 1 with id NULL: a communicator over this engine's devices alone
 * (ncclCommInitAll; also at one device).  Replaces an earlier communicator. */
int cls_comm_unique_id(void* id128);
int cls_comm_init(cls_engine* e, uint32_t n_procs, uint32_t proc, const void* id128);
/* Ranks of the engine's communicator (0: none) and its first device's rank. */
int cls_comm_info(cls_engine* e, uint32_t* n_ranks, uint32_t* rank0);

/* ---- offline compilation (no device needed) -----------------------------
 * Compiles an ACL exactly as cls_table_put does and writes the IPv4 device
 * layouts into `blob`: a cls_image_v4_header followed by the classifier image,
 * the slot->rule map and the linear rules.  With cap too small (or blob NULL)
 * only *need is set.  Used for inspection and CPU-side verification of the
 * compiler.
 */
typedef struct cls_image_v4_header {
    uint32_t magic;            /* 0x434C5334 "CLS4" */
    uint32_t version;          /* 4 (CLS_ABI_VERSION 3) */
    uint32_t n_rules, n_lin, has_cls;
    uint32_t img_bytes, off_bounds, off_iclass, off_cells, off_lists, off_tmpl;
    uint32_t n_bounds, search_top, n_classes, n_tmpl, n_list_entries, n_ctr, lds_bytes;
    uint32_t off_image, off_ctr_rule, off_lin;   /* byte offsets inside the blob */
    uint32_t total_bytes;
    uint32_t mode;             /* source lookup: 0 interval search, 1 hash LPM, 4 trie */
    uint32_t default_class;    /* hash LPM: class when no hashed prefix matches */
    uint32_t n_hash;           /* hashed prefix lengths (ascending) */
    uint32_t hash_mask[3], hash_shift[3], hash_cap[3], off_hash[3];
    uint32_t list_mode;        /* candidate lists: 0 template scan, 1 bit vectors,
                                  2 bit vectors with global port classes,
                                  3 port-filtered sublists (radix port classes),
                                  4 port-filtered sublists (hashed port classes),
                                  5, 6: 4, 3 with wide cells in global memory (off_gcells) */
    uint32_t off_bv, bv_steps_d, bv_steps_p;
    uint32_t off_ptop;         /* list modes 2, 3: port radix at 0 (256 x u32 window address,
                                  then u8 windows of class per port) */
    uint32_t n_pclass;         /* list modes 2, 3: global port classes */
    uint32_t bv_wide;          /* some bit-vector list has more than 16 entries */
    uint32_t row_bytes;        /* a class's 4 cells (TCP, UDP, ICMP, other protocols) at
                                  off_cells + class x row_bytes */
    uint32_t default_row;      /* hash LPM: cell row of default_class (hash entries hold rows) */
    uint32_t hash_mul[3];      /* hash LPM: p = key x mul; h0 = p >> shift, h1 = next log2(cap) bits */
    uint32_t port_mul, port_mask4, port_dflt;  /* list mode 4: e = u32 at byte mulhi(port, mul) &
                                  mask4, class x 4 = (e & 0xFFFF) == port ? e >> 16 : port_dflt */
    uint32_t n_hot, off_hot;   /* per-lane counter rows of the hot slots (LDS offsets) */
    uint32_t n_lctr;           /* slots counted in LDS (the rest: global counters) */
    uint32_t ctr16;            /* LDS slot counters are u16 (else u32) */
    uint32_t swap;             /* 1: classes keyed on the DESTINATION address -- the image sees
                                  packets with src and dst exchanged */
    uint32_t off_other;        /* blob offset of the OTHER image (protocols > 2: one cell per
                                  class, interval search, template scan; magic 0x434C534F "CLSO",
                                  its slots numbered after this image's), 0 if none */
    uint32_t off_trie;         /* mode 4 (source trie): level 1 (256 u32 by src >> 24: node byte
                                  address), nodes (256 u32 by bits 16..23: leaf byte address << 4
                                  | depth), leaves (2^depth u32 {key | class << 16}) */
    uint32_t trie_depth;       /* deepest leaf of the trie */
    uint32_t off_gcells;       /* list modes 5, 6 (4, 3 with wide cells): blob offset of the
                                  cells, uint2 {pointer table byte address, counter base} per
                                  (class, protocol); n_gcells u32 words */
    uint32_t n_gcells;
} cls_image_v4_header;
int cls_compile_v4(const cls_rule* rules, uint32_t n_rules, void* blob, uint64_t cap,
                   uint64_t* need, const char* options);   /* "key=value,..." (cls_engine_set_option's compiler keys) or NULL */
/* Whether the library has a classify kernel for an image of source lookup
 * `mode` and `list_mode` (cls_image_v4_header), LDS-resident or in global
 * memory; rep16: the 16-byte core.  CLS_OK, or CLS_E_INVAL for a combination
 * no kernel implements -- cls_table_put / cls_acl_put refuse such an image
 * with CLS_E_INVAL instead of launching another variant's kernel on it. */
int cls_image_kernel(uint32_t mode, uint32_t list_mode, int lds_resident, int rep16);
/* Diagnostics (CPU verification): the bitmap form cls_connect_batch gives a
 * linear IPv4 ACL (per-ACL interval tables of source, destination and each
 * protocol's destination port, one rule bit row per interval), built from
 * `rules` and evaluated on the host for n IPv4 packets: evalACL's ACLAction
 * and the terminating rule (n_rules: default DENY) per packet. */
int cls_conn_bitmap_eval(const cls_rule* rules, uint32_t n_rules, const uint32_t* src, const uint32_t* dst,
                         const uint16_t* dport, const uint8_t* proto, uint64_t n, uint8_t* res_out,
                         uint32_t* rule_out);

/* The 16-byte layout's compiled form (what cls_classify runs for CLS_AF_V16
 * batches): both address families are mapped to 32-bit representatives by a
 * front end -- per side (0 src, 1 dst) fe_top 16-B keys at image offset
 * fe_key (interval start - 1 as u64 hi, u64 lo in address order; padding all
 * ones) and fe_n u32 representatives at fe_val -- and `core` is the IPv4
 * classifier over the rules restated on representatives (magic 0x434C3136
 * "CL16"; its linear rules are in representative space too).  Returns
 * CLS_E_INVAL when the table has no 16-byte classifier.  Option pair4=1 (as
 * cls_compile_v4's): the connection pair launch's image instead, in the main
 * image's orientation -- the same front-end tables and source-search
 * trailer, a core of four cells per class (the fourth for protocols > 2)
 * with slots of its own, and no OTHER image (off_other 0).
 */
typedef struct cls_image_v16_header {
    cls_image_v4_header core;
    uint32_t fe_key[2], fe_val[2], fe_top[2], fe_n[2];
    /* src_mode 1 (every source prefix a host route): the source side is two
     * cuckoo hashes straight to class rows -- IPv4-mapped: {key, row} 8-B
     * entries at h4 (2 x cap4), key = address bytes 12-15 as a little-endian
     * word, h = key x mul4; IPv6: 16-B keys at k6 and u32 rows at r6 (2 x
     * cap6 slots), h = (w0 x fold0 ^ w1 x fold1 ^ w2 x fold2 ^ w3) x mul6;
     * table 0 slot = h >> (32 - L), table 1 slot = (h >> (32 - 2L)) & (cap - 1).
     * The source interval table (keys, reps at src_search_val) is then not
     * in the image but at blob offset off_src_search (the protocol > 2 path). */
    uint32_t src_mode, h4, cap4, mul4, k6, r6, cap6, mul6, fold[3], dflt_row[2];
    uint32_t off_src_search, src_search_val;
    /* fe_k8[s]: side s's keys are 8 B, key8(start) - 1 with key8(x) = hi64 == 0 ?
     * min(lo64, 2^48) : 2^48 + min(hi64, 2^64 - 1 - 2^48) (exact when every
     * start has hi64 = 0 and lo64 <= 2^48, or lo64 = 0) */
    uint32_t fe_k8[2];
    /* src_mode 2 (sources not all host routes, many IPv4 intervals): an
     * IPv4-mapped source's row from the trie over its IPv4 word at the core
     * header's off_trie / trie_depth (leaf entries carry the core's class);
     * any other source's row from the side-0 search (fe_key[0] ...), whose
     * table holds only the non-IPv4 intervals and rows as values.  src_mode
     * 1 and 2: the source interval table at off_src_search has
     * src_search_top keys (8 B when src_search_k8). */
    uint32_t src_search_top, src_search_k8;
} cls_image_v16_header;
int cls_compile_v16(const cls_rule* rules, uint32_t n_rules, void* blob, uint64_t cap,
                    uint64_t* need, const char* options);

#ifdef __cplusplus
}
#endif
#endif /* CONTIVCLS_H */
