/*
 * contivcls_go.h -- cgo shims of the C ABI (contivcls.h) for a Go host as
 * old as the reference's Go 1.9.x (/root/reference .travis.yml:7-8).
 *
 * cgo (Go >= 1.6) lets C receive a pointer to Go memory only if that memory
 * holds no Go pointers.  The ABI's packet and connection records
 * (cls_pkt_soa, cls_conn_soa) hold array pointers, so a Go value of them
 * that points at Go slices may not be passed -- Go 1.21's runtime.Pinner is
 * the newer way around that.  These shims take each slice base as a scalar
 * argument instead (a pointer to pointer-free Go memory, valid for the call)
 * and build the records on the C stack, so the Go side needs neither
 * runtime.Pinner nor unsafe.Slice.  Every shim is one ABI call; the engine
 * keeps no caller pointer after it returns (contivcls.h conventions).
 *
 * Static inline: the header is compiled into the cgo preamble (and into
 * go/shimtest/shimtest.c, which exercises exactly these functions through
 * libcontivcls.so on the GPU, tests/test_gpu_go_shims.py).
 */
#ifndef CONTIVCLS_GO_H
#define CONTIVCLS_GO_H

#include <string.h>

#include "contivcls.h"

/* cls_engine_create over devices[0 .. n) (n 1: one device, devices[0] may be
 * -1 for the current one).  Replaces NewMockACLEngine (aclengine_mock.go:124). */
static inline int clsg_engine_create(const int* devices, uint32_t n, cls_engine** out) {
    cls_config c;
    memset(&c, 0, sizeof c);
    c.device = n ? devices[0] : -1;
    if (n > 1) {
        c.n_devices = n;
        c.devices = devices;
    }
    return cls_engine_create(&c, out);
}

/* cls_classify of an IPv4 batch (host-order addresses): evalACL per packet
 * (aclengine_mock.go:473-668) and the table's hit counters. */
static inline int clsg_classify_v4(cls_engine* e, uint32_t table_id, const uint32_t* src4, const uint32_t* dst4,
                                   const uint16_t* dport, const uint8_t* proto, uint64_t n, uint8_t* verdict,
                                   uint64_t* counters, uint32_t flags) {
    cls_pkt_soa p;
    memset(&p, 0, sizeof p);
    p.af = CLS_AF_V4;
    p.src4 = src4;
    p.dst4 = dst4;
    p.dport = dport;
    p.proto = proto;
    return cls_classify(e, table_id, &p, n, verdict, counters, flags, NULL);
}

/* cls_classify of a 16-byte batch (n x 16 network-order bytes per address;
 * IPv4 as IPv4-mapped, Go's net.IP.To16). */
/* cls_classify_rules over an IPv4 batch: each packet's ACLAction and terminating rule. */
static inline int clsg_classify_rules_v4(cls_engine* e, uint32_t table_id, const uint32_t* src4, const uint32_t* dst4,
                                         const uint16_t* dport, const uint8_t* proto, uint64_t n, uint8_t* verdict,
                                         uint32_t* rules) {
    cls_pkt_soa p;
    memset(&p, 0, sizeof p);
    p.af = CLS_AF_V4;
    p.src4 = src4;
    p.dst4 = dst4;
    p.dport = dport;
    p.proto = proto;
    return cls_classify_rules(e, table_id, &p, n, verdict, rules, 0, NULL);
}

static inline int clsg_classify_v16(cls_engine* e, uint32_t table_id, const uint8_t* src16, const uint8_t* dst16,
                                    const uint16_t* dport, const uint8_t* proto, uint64_t n, uint8_t* verdict,
                                    uint64_t* counters, uint32_t flags) {
    cls_pkt_soa p;
    memset(&p, 0, sizeof p);
    p.af = CLS_AF_V16;
    p.src16 = src16;
    p.dst16 = dst16;
    p.dport = dport;
    p.proto = proto;
    return cls_classify(e, table_id, &p, n, verdict, counters, flags, NULL);
}

/* cls_connect_batch of IPv4 connections: testConnection per connection
 * (aclengine_mock.go:394-471) between interface ids (cls_if_id). */
static inline int clsg_connect_v4(cls_engine* e, const uint32_t* src_if, const uint32_t* dst_if, const uint32_t* src4,
                                  const uint32_t* dst4, const uint16_t* sport, const uint16_t* dport,
                                  const uint8_t* proto, uint64_t n, uint8_t* out, uint32_t flags) {
    cls_conn_soa c;
    memset(&c, 0, sizeof c);
    c.pkt.af = CLS_AF_V4;
    c.pkt.src4 = src4;
    c.pkt.dst4 = dst4;
    c.pkt.sport = sport;
    c.pkt.dport = dport;
    c.pkt.proto = proto;
    c.src_if = src_if;
    c.dst_if = dst_if;
    return cls_connect_batch(e, &c, n, out, flags, NULL);
}

/* cls_connect_batch of 16-byte connections. */
static inline int clsg_connect_v16(cls_engine* e, const uint32_t* src_if, const uint32_t* dst_if, const uint8_t* src16,
                                   const uint8_t* dst16, const uint16_t* sport, const uint16_t* dport,
                                   const uint8_t* proto, uint64_t n, uint8_t* out, uint32_t flags) {
    cls_conn_soa c;
    memset(&c, 0, sizeof c);
    c.pkt.af = CLS_AF_V16;
    c.pkt.src16 = src16;
    c.pkt.dst16 = dst16;
    c.pkt.sport = sport;
    c.pkt.dport = dport;
    c.pkt.proto = proto;
    c.src_if = src_if;
    c.dst_if = dst_if;
    return cls_connect_batch(e, &c, n, out, flags, NULL);
}

/* cls_connect_rules of IPv4 connections: the ConnectionAction (out, may be
 * NULL) and the four evalACL calls' terminating rules (rules[4 i + k], -1: no
 * call) per connection. */
static inline int clsg_connect_rules_v4(cls_engine* e, const uint32_t* src_if, const uint32_t* dst_if,
                                        const uint32_t* src4, const uint32_t* dst4, const uint16_t* sport,
                                        const uint16_t* dport, const uint8_t* proto, uint64_t n, uint8_t* out,
                                        int32_t* rules, uint32_t flags) {
    cls_conn_soa c;
    memset(&c, 0, sizeof c);
    c.pkt.af = CLS_AF_V4;
    c.pkt.src4 = src4;
    c.pkt.dst4 = dst4;
    c.pkt.sport = sport;
    c.pkt.dport = dport;
    c.pkt.proto = proto;
    c.src_if = src_if;
    c.dst_if = dst_if;
    return cls_connect_rules(e, &c, n, out, rules, flags, NULL);
}

/* cls_connect_rules of 16-byte connections. */
static inline int clsg_connect_rules_v16(cls_engine* e, const uint32_t* src_if, const uint32_t* dst_if,
                                         const uint8_t* src16, const uint8_t* dst16, const uint16_t* sport,
                                         const uint16_t* dport, const uint8_t* proto, uint64_t n, uint8_t* out,
                                         int32_t* rules, uint32_t flags) {
    cls_conn_soa c;
    memset(&c, 0, sizeof c);
    c.pkt.af = CLS_AF_V16;
    c.pkt.src16 = src16;
    c.pkt.dst16 = dst16;
    c.pkt.sport = sport;
    c.pkt.dport = dport;
    c.pkt.proto = proto;
    c.src_if = src_if;
    c.dst_if = dst_if;
    return cls_connect_rules(e, &c, n, out, rules, flags, NULL);
}

/* cls_reach_matrix over IPv4 endpoints: testConnection for every (probe,
 * source, destination) cell of n endpoints x n_probes probes -- what the
 * reference answers by looping ConnectionPodToPod over pods and ports
 * (aclengine_mock.go:243-300).  Host outputs; verdict (n_probes x n x n),
 * hist (n_probes x 4) and allow (n_probes x n) may each be NULL (not all;
 * verdict NULL needs CLS_F_NO_VERDICT). */
static inline int clsg_reach_matrix_v4(cls_engine* e, const uint32_t* if_id, const uint32_t* addr4, uint32_t n,
                                       const uint8_t* proto, const uint16_t* sport, const uint16_t* dport,
                                       uint32_t n_probes, uint8_t* verdict, uint64_t* hist, uint32_t* allow,
                                       uint32_t flags) {
    cls_reach_spec r;
    memset(&r, 0, sizeof r);
    r.af = CLS_AF_V4;
    r.n_endpoints = n;
    r.if_id = if_id;
    r.addr4 = addr4;
    r.n_probes = n_probes;
    r.proto = proto;
    r.sport = sport;
    r.dport = dport;
    return cls_reach_matrix(e, &r, verdict, hist, allow, flags, NULL);
}

/* cls_reach_matrix over 16-byte endpoints (n x 16 network-order bytes). */
static inline int clsg_reach_matrix_v16(cls_engine* e, const uint32_t* if_id, const uint8_t* addr16, uint32_t n,
                                        const uint8_t* proto, const uint16_t* sport, const uint16_t* dport,
                                        uint32_t n_probes, uint8_t* verdict, uint64_t* hist, uint32_t* allow,
                                        uint32_t flags) {
    cls_reach_spec r;
    memset(&r, 0, sizeof r);
    r.af = CLS_AF_V16;
    r.n_endpoints = n;
    r.if_id = if_id;
    r.addr16 = addr16;
    r.n_probes = n_probes;
    r.proto = proto;
    r.sport = sport;
    r.dport = dport;
    return cls_reach_matrix(e, &r, verdict, hist, allow, flags, NULL);
}

/* cls_reach_diff over IPv4 endpoints: the matrix of clsg_reach_matrix_v4's
 * arguments against the baseline `base` (n_probes x n x n, of an earlier
 * call).  Host arrays; verdict (may be base: in place), hist, allow, changes
 * (cap records of 16 bytes: probe, src, dst as u32, then was, now and two zero
 * bytes; needs n_changes), n_changes (1), trans (n_probes x 16) and changed
 * (n_probes x n) may each be NULL, but not all of the last four. */
static inline int clsg_reach_diff_v4(cls_engine* e, const uint32_t* if_id, const uint32_t* addr4, uint32_t n,
                                     const uint8_t* proto, const uint16_t* sport, const uint16_t* dport,
                                     uint32_t n_probes, const uint8_t* base, uint8_t* verdict, uint64_t* hist,
                                     uint32_t* allow, void* changes, uint64_t cap, uint64_t* n_changes,
                                     uint64_t* trans, uint32_t* changed, uint32_t flags) {
    cls_reach_spec r;
    cls_reach_diff_out o;
    memset(&r, 0, sizeof r);
    r.af = CLS_AF_V4;
    r.n_endpoints = n;
    r.if_id = if_id;
    r.addr4 = addr4;
    r.n_probes = n_probes;
    r.proto = proto;
    r.sport = sport;
    r.dport = dport;
    memset(&o, 0, sizeof o);
    o.verdict_out = verdict;
    o.hist_out = hist;
    o.allow_out = allow;
    o.changes = (cls_reach_change*)changes;
    o.cap = cap;
    o.n_changes = n_changes;
    o.trans_out = trans;
    o.changed_out = changed;
    return cls_reach_diff(e, &r, base, &o, flags, NULL);
}

/* cls_reach_diff over 16-byte endpoints (n x 16 network-order bytes). */
static inline int clsg_reach_diff_v16(cls_engine* e, const uint32_t* if_id, const uint8_t* addr16, uint32_t n,
                                      const uint8_t* proto, const uint16_t* sport, const uint16_t* dport,
                                      uint32_t n_probes, const uint8_t* base, uint8_t* verdict, uint64_t* hist,
                                      uint32_t* allow, void* changes, uint64_t cap, uint64_t* n_changes,
                                      uint64_t* trans, uint32_t* changed, uint32_t flags) {
    cls_reach_spec r;
    cls_reach_diff_out o;
    memset(&r, 0, sizeof r);
    r.af = CLS_AF_V16;
    r.n_endpoints = n;
    r.if_id = if_id;
    r.addr16 = addr16;
    r.n_probes = n_probes;
    r.proto = proto;
    r.sport = sport;
    r.dport = dport;
    memset(&o, 0, sizeof o);
    o.verdict_out = verdict;
    o.hist_out = hist;
    o.allow_out = allow;
    o.changes = (cls_reach_change*)changes;
    o.cap = cap;
    o.n_changes = n_changes;
    o.trans_out = trans;
    o.changed_out = changed;
    return cls_reach_diff(e, &r, base, &o, flags, NULL);
}

/* cls_reach_ports over IPv4 endpoints: per-pair port ranges over all 65,536
 * destination ports for one protocol and source port.  Host arrays; ranges
 * (cap records of 16 bytes: src, dst as u32, port_lo, port_hi as u16, the
 * action and three zero bytes; needs n_ranges), n_ranges (1), runs and
 * allow_ports (n x n each) and hist (4) may each be NULL, but not all;
 * n_classes (1) may be NULL. */
static inline int clsg_reach_ports_v4(cls_engine* e, const uint32_t* if_id, const uint32_t* addr4, uint32_t n,
                                      uint8_t proto, uint16_t sport, void* ranges, uint64_t cap, uint64_t* n_ranges,
                                      uint32_t* runs, uint32_t* allow_ports, uint64_t* hist, uint32_t* n_classes,
                                      uint32_t flags) {
    cls_reach_spec r;
    cls_reach_ports_out o;
    memset(&r, 0, sizeof r);
    r.af = CLS_AF_V4;
    r.n_endpoints = n;
    r.if_id = if_id;
    r.addr4 = addr4;
    r.n_probes = 1;
    r.proto = &proto;
    r.sport = &sport;
    memset(&o, 0, sizeof o);
    o.ranges = (cls_port_range*)ranges;
    o.cap = cap;
    o.n_ranges = n_ranges;
    o.runs_out = runs;
    o.allow_ports_out = allow_ports;
    o.hist_out = hist;
    o.n_classes = n_classes;
    return cls_reach_ports(e, &r, &o, flags, NULL);
}

/* cls_reach_ports over 16-byte endpoints (n x 16 network-order bytes). */
static inline int clsg_reach_ports_v16(cls_engine* e, const uint32_t* if_id, const uint8_t* addr16, uint32_t n,
                                       uint8_t proto, uint16_t sport, void* ranges, uint64_t cap, uint64_t* n_ranges,
                                       uint32_t* runs, uint32_t* allow_ports, uint64_t* hist, uint32_t* n_classes,
                                       uint32_t flags) {
    cls_reach_spec r;
    cls_reach_ports_out o;
    memset(&r, 0, sizeof r);
    r.af = CLS_AF_V16;
    r.n_endpoints = n;
    r.if_id = if_id;
    r.addr16 = addr16;
    r.n_probes = 1;
    r.proto = &proto;
    r.sport = &sport;
    memset(&o, 0, sizeof o);
    o.ranges = (cls_port_range*)ranges;
    o.cap = cap;
    o.n_ranges = n_ranges;
    o.runs_out = runs;
    o.allow_ports_out = allow_ports;
    o.hist_out = hist;
    o.n_classes = n_classes;
    return cls_reach_ports(e, &r, &o, flags, NULL);
}

/* cls_reach_hops over IPv4 endpoints: the multi-hop closure of the matrix of
 * clsg_reach_matrix_v4's arguments, evaluated on the device and never stored,
 * paths of at most max_hops edges (0: 254).  Host arrays; hops (n x n bytes),
 * reach and exposed (n each), level (256) and closure (n x (n + 63) / 64) may
 * each be NULL, but not all. */
static inline int clsg_reach_hops_v4(cls_engine* e, const uint32_t* if_id, const uint32_t* addr4, uint32_t n,
                                     const uint8_t* proto, const uint16_t* sport, const uint16_t* dport,
                                     uint32_t n_probes, uint32_t max_hops, uint8_t* hops, uint32_t* reach,
                                     uint32_t* exposed, uint64_t* level, uint64_t* closure, uint32_t flags) {
    cls_reach_spec r;
    cls_reach_hops_out o;
    memset(&r, 0, sizeof r);
    r.af = CLS_AF_V4;
    r.n_endpoints = n;
    r.if_id = if_id;
    r.addr4 = addr4;
    r.n_probes = n_probes;
    r.proto = proto;
    r.sport = sport;
    r.dport = dport;
    memset(&o, 0, sizeof o);
    o.hops_out = hops;
    o.reach_out = reach;
    o.exposed_out = exposed;
    o.level_out = level;
    o.closure_out = closure;
    return cls_reach_hops(e, &r, NULL, max_hops, &o, flags, NULL);
}

/* cls_reach_hops over 16-byte endpoints (n x 16 network-order bytes). */
static inline int clsg_reach_hops_v16(cls_engine* e, const uint32_t* if_id, const uint8_t* addr16, uint32_t n,
                                      const uint8_t* proto, const uint16_t* sport, const uint16_t* dport,
                                      uint32_t n_probes, uint32_t max_hops, uint8_t* hops, uint32_t* reach,
                                      uint32_t* exposed, uint64_t* level, uint64_t* closure, uint32_t flags) {
    cls_reach_spec r;
    cls_reach_hops_out o;
    memset(&r, 0, sizeof r);
    r.af = CLS_AF_V16;
    r.n_endpoints = n;
    r.if_id = if_id;
    r.addr16 = addr16;
    r.n_probes = n_probes;
    r.proto = proto;
    r.sport = sport;
    r.dport = dport;
    memset(&o, 0, sizeof o);
    o.hops_out = hops;
    o.reach_out = reach;
    o.exposed_out = exposed;
    o.level_out = level;
    o.closure_out = closure;
    return cls_reach_hops(e, &r, NULL, max_hops, &o, flags, NULL);
}

/* cls_reach_classes over IPv4 endpoints: the classes of endpoints that the
 * matrix of clsg_reach_matrix_v4's arguments cannot tell apart, evaluated on
 * the device.  Host arrays; classes (n) or n_classes is required; rep and
 * size (class_cap each), self_ (n_probes x class_cap) and quot (n_probes x
 * class_cap x class_cap) are written, dense in C, only when C <= class_cap;
 * verdict (n_probes x n x n) and rounds may be NULL.  Returns with the result
 * complete. */
static inline int clsg_reach_classes_v4(cls_engine* e, const uint32_t* if_id, const uint32_t* addr4, uint32_t n,
                                         const uint8_t* proto, const uint16_t* sport, const uint16_t* dport,
                                         uint32_t n_probes, uint32_t* classes, uint32_t* n_classes, uint64_t class_cap,
                                         uint32_t* rep, uint32_t* size, uint8_t* self_, uint8_t* quot,
                                         uint8_t* verdict, uint32_t* rounds, uint32_t flags) {
    cls_reach_spec r;
    cls_reach_classes_out o;
    memset(&r, 0, sizeof r);
    r.af = CLS_AF_V4;
    r.n_endpoints = n;
    r.if_id = if_id;
    r.addr4 = addr4;
    r.n_probes = n_probes;
    r.proto = proto;
    r.sport = sport;
    r.dport = dport;
    memset(&o, 0, sizeof o);
    o.class_out = classes;
    o.n_classes = n_classes;
    o.class_cap = class_cap;
    o.rep_out = rep;
    o.size_out = size;
    o.self_out = self_;
    o.quot_out = quot;
    o.verdict_out = verdict;
    o.rounds = rounds;
    return cls_reach_classes(e, &r, NULL, &o, flags, NULL);
}

/* cls_reach_classes over 16-byte endpoints (n x 16 network-order bytes). */
static inline int clsg_reach_classes_v16(cls_engine* e, const uint32_t* if_id, const uint8_t* addr16, uint32_t n,
                                         const uint8_t* proto, const uint16_t* sport, const uint16_t* dport,
                                         uint32_t n_probes, uint32_t* classes, uint32_t* n_classes, uint64_t class_cap,
                                         uint32_t* rep, uint32_t* size, uint8_t* self_, uint8_t* quot,
                                         uint8_t* verdict, uint32_t* rounds, uint32_t flags) {
    cls_reach_spec r;
    cls_reach_classes_out o;
    memset(&r, 0, sizeof r);
    r.af = CLS_AF_V16;
    r.n_endpoints = n;
    r.if_id = if_id;
    r.addr16 = addr16;
    r.n_probes = n_probes;
    r.proto = proto;
    r.sport = sport;
    r.dport = dport;
    memset(&o, 0, sizeof o);
    o.class_out = classes;
    o.n_classes = n_classes;
    o.class_cap = class_cap;
    o.rep_out = rep;
    o.size_out = size;
    o.self_out = self_;
    o.quot_out = quot;
    o.verdict_out = verdict;
    o.rounds = rounds;
    return cls_reach_classes(e, &r, NULL, &o, flags, NULL);
}

/* cls_reach_external over IPv4 endpoints: per-endpoint remote address ranges
 * over all of IPv4 through the interface ext_if, for p probes and the
 * directions of dirs (CLS_EXT_EGRESS | CLS_EXT_INGRESS; d of them).  Host
 * arrays; ranges (cap records of 16 bytes: src as u32, probe as u16, dir and
 * action as u8, addr_lo and addr_hi as u32; needs n_ranges), n_ranges (1),
 * runs (d x p x n u32), allow_addrs (d x p x n u64) and hist (d x p x 4 u64)
 * may each be NULL, but not all; n_classes (1) may be NULL. */
static inline int clsg_reach_external_v4(cls_engine* e, const uint32_t* if_id, const uint32_t* addr4, uint32_t n,
                                         const uint8_t* proto, const uint16_t* sport, const uint16_t* dport,
                                         uint32_t p, uint32_t ext_if, uint32_t dirs, void* ranges, uint64_t cap,
                                         uint64_t* n_ranges, uint32_t* runs, uint64_t* allow_addrs, uint64_t* hist,
                                         uint32_t* n_classes, uint32_t flags) {
    cls_reach_spec r;
    cls_reach_ext_out o;
    memset(&r, 0, sizeof r);
    r.af = CLS_AF_V4;
    r.n_endpoints = n;
    r.if_id = if_id;
    r.addr4 = addr4;
    r.n_probes = p;
    r.proto = proto;
    r.sport = sport;
    r.dport = dport;
    memset(&o, 0, sizeof o);
    o.ranges = (cls_addr_range*)ranges;
    o.cap = cap;
    o.n_ranges = n_ranges;
    o.runs_out = runs;
    o.allow_addrs_out = allow_addrs;
    o.hist_out = hist;
    o.n_classes = n_classes;
    return cls_reach_external(e, &r, ext_if, dirs, &o, flags, NULL);
}

/* cls_reach_external over 16-byte endpoints (n x 16 network-order bytes); the
 * remote addresses are the IPv4-mapped ::ffff:a. */
static inline int clsg_reach_external_v16(cls_engine* e, const uint32_t* if_id, const uint8_t* addr16, uint32_t n,
                                          const uint8_t* proto, const uint16_t* sport, const uint16_t* dport,
                                          uint32_t p, uint32_t ext_if, uint32_t dirs, void* ranges, uint64_t cap,
                                          uint64_t* n_ranges, uint32_t* runs, uint64_t* allow_addrs, uint64_t* hist,
                                          uint32_t* n_classes, uint32_t flags) {
    cls_reach_spec r;
    cls_reach_ext_out o;
    memset(&r, 0, sizeof r);
    r.af = CLS_AF_V16;
    r.n_endpoints = n;
    r.if_id = if_id;
    r.addr16 = addr16;
    r.n_probes = p;
    r.proto = proto;
    r.sport = sport;
    r.dport = dport;
    memset(&o, 0, sizeof o);
    o.ranges = (cls_addr_range*)ranges;
    o.cap = cap;
    o.n_ranges = n_ranges;
    o.runs_out = runs;
    o.allow_addrs_out = allow_addrs;
    o.hist_out = hist;
    o.n_classes = n_classes;
    return cls_reach_external(e, &r, ext_if, dirs, &o, flags, NULL);
}

/* cls_table_cover of one table over the IPv4 packet space, IPv4 layout: which
 * rules no packet terminates at and a witness packet for each of the others.
 * Host arrays over the table's r rules and the default DENY at index r; live
 * (r + 1 u8), witness (r + 1 records of 16 bytes: src and dst as u32, dport as
 * u16, proto and live as u8, a zero u32), cells (r + 1 u64) and n_dead (1) may
 * each be NULL, but not all; n_cells (1) and dims (4: Ks, Kd, Kt, Ku) may be
 * NULL. */
static inline int clsg_table_cover_v4(cls_engine* e, uint32_t table_id, uint8_t* live, void* witness, uint64_t* cells,
                                      uint32_t* n_dead, uint64_t* n_cells, uint32_t* dims, uint32_t flags) {
    cls_cover_out o;
    memset(&o, 0, sizeof o);
    o.live_out = live;
    o.witness_out = (cls_cover_witness*)witness;
    o.cells_out = cells;
    o.n_dead = n_dead;
    o.n_cells = n_cells;
    o.dims = dims;
    return cls_table_cover(e, table_id, CLS_AF_V4, &o, flags, NULL);
}

/* The same sweep through the 16-byte classifier: the packets are the
 * IPv4-mapped ::ffff:src / ::ffff:dst. */
static inline int clsg_table_cover_v16(cls_engine* e, uint32_t table_id, uint8_t* live, void* witness, uint64_t* cells,
                                       uint32_t* n_dead, uint64_t* n_cells, uint32_t* dims, uint32_t flags) {
    cls_cover_out o;
    memset(&o, 0, sizeof o);
    o.live_out = live;
    o.witness_out = (cls_cover_witness*)witness;
    o.cells_out = cells;
    o.n_dead = n_dead;
    o.n_cells = n_cells;
    o.dims = dims;
    return cls_table_cover(e, table_id, CLS_AF_V16, &o, flags, NULL);
}

/* cls_table_diff of two tables over the IPv4 packet space, IPv4 layout: the
 * packets whose ACLAction differs between table_a and table_b.  Host arrays:
 * n_diff (1), pairs (16: cells per (was, now)), first (one 16-byte
 * cls_cover_witness), cells_a / wit_a over table_a's rules and its default
 * DENY, cells_b / wit_b over table_b's, rec (rec_cap 32-byte cls_tdiff_rec)
 * with n_rec (1: the total, also above rec_cap).  Each may be NULL, but not
 * all, and rec needs n_rec; n_cells (1) and dims (4: the joint Ks, Kd, Kt, Ku)
 * may be NULL. */
static inline int clsg_table_diff_af(cls_engine* e, uint32_t af, uint32_t table_a, uint32_t table_b, uint64_t* n_diff,
                                     uint64_t* pairs, void* first, uint64_t* cells_a, void* wit_a, uint64_t* cells_b,
                                     void* wit_b, void* rec, uint64_t rec_cap, uint64_t* n_rec, uint64_t* n_cells,
                                     uint32_t* dims, uint32_t flags) {
    cls_tdiff_out o;
    memset(&o, 0, sizeof o);
    o.n_diff = n_diff;
    o.pairs_out = pairs;
    o.first_out = (cls_cover_witness*)first;
    o.cells_a = cells_a;
    o.wit_a = (cls_cover_witness*)wit_a;
    o.cells_b = cells_b;
    o.wit_b = (cls_cover_witness*)wit_b;
    o.rec_out = (cls_tdiff_rec*)rec;
    o.rec_cap = rec_cap;
    o.n_rec = n_rec;
    o.n_cells = n_cells;
    o.dims = dims;
    return cls_table_diff(e, table_a, table_b, af, &o, flags, NULL);
}
static inline int clsg_table_diff_v4(cls_engine* e, uint32_t table_a, uint32_t table_b, uint64_t* n_diff,
                                     uint64_t* pairs, void* first, uint64_t* cells_a, void* wit_a, uint64_t* cells_b,
                                     void* wit_b, void* rec, uint64_t rec_cap, uint64_t* n_rec, uint64_t* n_cells,
                                     uint32_t* dims, uint32_t flags) {
    return clsg_table_diff_af(e, CLS_AF_V4, table_a, table_b, n_diff, pairs, first, cells_a, wit_a, cells_b, wit_b, rec,
                              rec_cap, n_rec, n_cells, dims, flags);
}

/* The same diff through the 16-byte classifier: the packets are the
 * IPv4-mapped ::ffff:src / ::ffff:dst. */
static inline int clsg_table_diff_v16(cls_engine* e, uint32_t table_a, uint32_t table_b, uint64_t* n_diff,
                                      uint64_t* pairs, void* first, uint64_t* cells_a, void* wit_a, uint64_t* cells_b,
                                      void* wit_b, void* rec, uint64_t rec_cap, uint64_t* n_rec, uint64_t* n_cells,
                                      uint32_t* dims, uint32_t flags) {
    return clsg_table_diff_af(e, CLS_AF_V16, table_a, table_b, n_diff, pairs, first, cells_a, wit_a, cells_b, wit_b,
                              rec, rec_cap, n_rec, n_cells, dims, flags);
}

/* cls_table_need of one table over the IPv4 packet space: the rules the list
 * can lose without changing a verdict.  skip: (r + 63) / 64 u64 words, bit k
 * set for a rule treated as deleted, or NULL.  Host arrays over the table's r
 * rules: need and free (r u8), first (r + 1 u64, index r the default DENY),
 * changed (r u64), witness (r records of 16 bytes: src and dst as u32, dport
 * as u16, proto and after as u8, fall as u32), counts (4 u32: rules per
 * CLS_NEED_* value) may each be NULL, but not all; n_cells (1) and dims (4:
 * Ks, Kd, Kt, Ku) may be NULL. */
static inline int clsg_table_need(cls_engine* e, uint32_t table_id, const uint64_t* skip, uint8_t* need, uint8_t* free_out,
                                  uint64_t* first, uint64_t* changed, void* witness, uint32_t* counts,
                                  uint64_t* n_cells, uint32_t* dims, uint32_t flags) {
    cls_need_out o;
    memset(&o, 0, sizeof o);
    o.need_out = need;
    o.free_out = free_out;
    o.first_out = first;
    o.changed_out = changed;
    o.witness_out = (cls_need_witness*)witness;
    o.counts = counts;
    o.n_cells = n_cells;
    o.dims = dims;
    return cls_table_need(e, table_id, skip, &o, flags, NULL);
}

/* The pinned host array of a batch field (CLS_BATCH_MIRROR), NULL if none:
 * C memory, so Go may keep it as a slice (Go 1.9: (*[1 << 32]T)(p)[:n:n]). */
static inline void* clsg_batch_mirror(cls_batch* b, uint32_t field) {
    void* p = NULL;
    return cls_batch_mirror(b, field, &p) == CLS_OK ? p : NULL;
}

/* The ABI version the shims were compiled against (a Go host checks it
 * against cls_abi_version() at start-up). */
static inline int clsg_abi_version(void) { return CLS_ABI_VERSION; }

#endif /* CONTIVCLS_GO_H */
