/*
 * reachext -- the Go binding's external-sweep shims (clsg_reach_external_v4 /
 * clsg_reach_external_v16, include/contivcls_go.h) driven from plain C the way
 * go/contivcls/contivcls.go's ReachExternal drives them;
 * tests/test_gpu_reach_ext.py checks its outputs against the Python call's.
 *
 * usage: reachext DIR 4|16
 *   DIR/acls.txt, DIR/ifs.txt, DIR/reach.bin   as reachtest's; the remote
 *   interface is the first of ifs.txt, both directions are swept
 * writes DIR/out_ext_ranges.bin (the 16-byte range records),
 * DIR/out_ext_n.bin (u64), DIR/out_ext_runs.bin (2 x p x n u32),
 * DIR/out_ext_allow.bin (2 x p x n u64), DIR/out_ext_hist.bin (2 x p x 4 u64)
 * and DIR/out_ext_k.bin (u32: the address classes).
 */
#define _POSIX_C_SOURCE 200809L   /* strdup */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "contivcls_go.h"

#define MAX_IFS 1024

static char dir[4096];

static void die(const char* what, cls_engine* e, int rc) {
    fprintf(stderr, "reachext: %s failed (rc %d): %s\n", what, rc, e ? cls_last_error(e) : "");
    exit(1);
}

static FILE* open_in(const char* name, const char* mode) {
    char p[4200];
    snprintf(p, sizeof p, "%s/%s", dir, name);
    FILE* f = fopen(p, mode);
    if (!f) {
        fprintf(stderr, "reachext: cannot open %s\n", p);
        exit(1);
    }
    return f;
}

static void* read_n(FILE* f, size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (!p || (bytes && fread(p, 1, bytes, f) != bytes)) {
        fprintf(stderr, "reachext: short input\n");
        exit(1);
    }
    return p;
}

static void write_out(const char* name, const void* p, size_t bytes) {
    FILE* f = open_in(name, "wb");
    if (bytes && fwrite(p, 1, bytes, f) != bytes) exit(1);
    fclose(f);
}

/* a network string: "-" (none) or "x" and its bytes in hex */
static char* dup_net(const char* s) {
    if (strcmp(s, "-") == 0) return NULL;
    const size_t n = strlen(s + 1) / 2;
    char* out = calloc(n + 1, 1);
    for (size_t i = 0; i < n; ++i) {
        unsigned v = 0;
        if (sscanf(s + 1 + 2 * i, "%2x", &v) != 1) exit(1);
        out[i] = (char)v;
    }
    return out;
}

int main(int argc, char** argv) {
    if (argc != 3 || (strcmp(argv[2], "4") != 0 && strcmp(argv[2], "16") != 0)) {
        fprintf(stderr, "usage: reachext DIR 4|16\n");
        return 2;
    }
    const int v16 = strcmp(argv[2], "16") == 0;
    snprintf(dir, sizeof dir, "%s", argv[1]);
    if (cls_abi_version() != clsg_abi_version()) {
        fprintf(stderr, "reachext: library ABI %d, shims %d\n", cls_abi_version(), clsg_abi_version());
        return 1;
    }
    int devs[1] = {0};
    cls_engine* e = NULL;
    int rc = clsg_engine_create(devs, 1, &e);
    if (rc != CLS_OK) die("clsg_engine_create", NULL, rc);

    /* ---- ACLs, installed as they are read --------------------------------- */
    uint32_t n_acls = 0;
    FILE* f = open_in("acls.txt", "r");
    char tag[16];
    while (fscanf(f, "%15s", tag) == 1) {
        char name[128], buf[256];
        char* in[16];
        char* out[16];
        uint32_t n_rules = 0, n_in = 0, n_out = 0;
        if (strcmp(tag, "acl") != 0) return 1;
        if (fscanf(f, "%127s %u %u", name, &n_rules, &n_in) != 3 || n_in > 16) return 1;
        for (uint32_t i = 0; i < n_in; ++i) {
            if (fscanf(f, "%255s", buf) != 1) return 1;
            in[i] = strdup(buf);
        }
        if (fscanf(f, "%u", &n_out) != 1 || n_out > 16) return 1;
        for (uint32_t i = 0; i < n_out; ++i) {
            if (fscanf(f, "%255s", buf) != 1) return 1;
            out[i] = strdup(buf);
        }
        cls_rule* rules = calloc(n_rules ? n_rules : 1, sizeof(cls_rule));
        for (uint32_t k = 0; k < n_rules; ++k) {
            cls_rule* r = &rules[k];
            char src[256], dst[256];
            if (fscanf(f, "%15s %u %d %u %u %u %u %u %u %u %u %u %u %u %u %255s %255s", tag, &r->flags,
                       &r->acl_action, &r->tcp_src_lo, &r->tcp_src_hi, &r->tcp_dst_lo, &r->tcp_dst_hi, &r->udp_src_lo,
                       &r->udp_src_hi, &r->udp_dst_lo, &r->udp_dst_hi, &r->icmp_code_first, &r->icmp_code_last,
                       &r->icmp_type_first, &r->icmp_type_last, src, dst) != 17)
                return 1;
            r->src_network = dup_net(src);
            r->dst_network = dup_net(dst);
        }
        rc = cls_acl_put(e, name, rules, n_rules, (const char* const*)in, n_in, (const char* const*)out, n_out);
        if (rc != CLS_OK) die("cls_acl_put", e, rc);
        ++n_acls;
    }
    fclose(f);
    if (n_acls == 0) return 1;

    /* ---- the sweep: endpoints and probes through the shims ------------------- */
    static char* ifn[MAX_IFS];
    uint32_t n_ifs = 0;
    f = open_in("ifs.txt", "r");
    char buf[256];
    while (n_ifs < MAX_IFS && fscanf(f, "%255s", buf) == 1) ifn[n_ifs++] = strdup(buf);
    fclose(f);
    uint32_t ids[MAX_IFS];
    for (uint32_t k = 0; k < n_ifs; ++k)
        if ((rc = cls_if_id(e, ifn[k], &ids[k])) != CLS_OK) die("cls_if_id", e, rc);
    f = open_in("reach.bin", "rb");
    uint32_t n = 0, p = 0;
    if (fread(&n, 4, 1, f) != 1 || fread(&p, 4, 1, f) != 1) return 1;
    uint32_t* ifs = read_n(f, (size_t)n * 4);
    void* addr = read_n(f, (size_t)n * (v16 ? 16 : 4));
    uint8_t* proto = read_n(f, p);
    uint16_t* sport = read_n(f, (size_t)p * 2);
    uint16_t* dport = read_n(f, (size_t)p * 2);
    fclose(f);
    for (uint32_t i = 0; i < n; ++i) {
        if (ifs[i] >= n_ifs) return 1;
        ifs[i] = ids[ifs[i]];
    }
    if (p < 1 || n_ifs < 1) return 1;
    const uint32_t ext = ids[0], dirs = CLS_EXT_EGRESS | CLS_EXT_INGRESS;
    const size_t lines = (size_t)2 * p * n, hw = (size_t)2 * p * 4;
    /* the ranges are counted first, then fetched */
    uint64_t n_ranges = ~(uint64_t)0, again = ~(uint64_t)0;
    uint32_t k = 0, k2 = 0;
    if (v16)
        rc = clsg_reach_external_v16(e, ifs, addr, n, proto, sport, dport, p, ext, dirs, NULL, 0, &n_ranges, NULL, NULL,
                                     NULL, &k, 0);
    else
        rc = clsg_reach_external_v4(e, ifs, addr, n, proto, sport, dport, p, ext, dirs, NULL, 0, &n_ranges, NULL, NULL,
                                    NULL, &k, 0);
    if (rc != CLS_OK) die("clsg_reach_external (count)", e, rc);
    if (n_ranges < lines || n_ranges > lines * k || k < 1) return 1;
    cls_addr_range* ranges = malloc((size_t)(n_ranges + 1) * sizeof(cls_addr_range));
    uint32_t* runs = malloc(lines ? lines * 4 : 4);
    uint64_t* allow = malloc(lines ? lines * 8 : 8);
    uint64_t* hist = malloc(hw * 8);
    memset(ranges, 0xEE, (size_t)(n_ranges + 1) * sizeof(cls_addr_range));
    memset(runs, 0xEE, lines ? lines * 4 : 4);
    memset(allow, 0xEE, lines ? lines * 8 : 8);
    memset(hist, 0xEE, hw * 8);
    if (v16) {
        rc = clsg_reach_external_v16(e, ifs, addr, n, proto, sport, dport, p, ext, dirs, ranges, n_ranges + 1, &again,
                                     runs, allow, hist, &k2, 0);
        if (rc != CLS_OK) die("clsg_reach_external_v16", e, rc);
    } else {
        rc = clsg_reach_external_v4(e, ifs, addr, n, proto, sport, dport, p, ext, dirs, ranges, n_ranges + 1, &again,
                                    runs, allow, hist, &k2, 0);
        if (rc != CLS_OK) die("clsg_reach_external_v4", e, rc);
    }
    /* the record past the total stays as it was */
    const unsigned char* past = (const unsigned char*)&ranges[n_ranges];
    for (size_t i = 0; i < sizeof(cls_addr_range); ++i)
        if (past[i] != 0xEE) return 1;
    /* a sweep without an output, without a direction, or with records but no
     * total or no room, is refused */
    if (again != n_ranges || k2 != k ||
        clsg_reach_external_v4(e, ifs, addr, n, proto, sport, dport, p, ext, dirs, NULL, 0, NULL, NULL, NULL, NULL, &k2,
                               0) != CLS_E_INVAL ||
        clsg_reach_external_v4(e, ifs, addr, n, proto, sport, dport, p, ext, 0, NULL, 0, &again, NULL, NULL, NULL, &k2,
                               0) != CLS_E_INVAL ||
        clsg_reach_external_v4(e, ifs, addr, n, proto, sport, dport, p, ext, dirs, ranges, n_ranges, NULL, runs, NULL,
                               NULL, &k2, 0) != CLS_E_INVAL ||
        clsg_reach_external_v4(e, ifs, addr, n, proto, sport, dport, p, ext, dirs, ranges, 0, &again, NULL, NULL, NULL,
                               &k2, 0) != CLS_E_INVAL) {
        fprintf(stderr, "reachext: a malformed sweep was accepted\n");
        return 1;
    }
    write_out("out_ext_ranges.bin", ranges, (size_t)n_ranges * sizeof(cls_addr_range));
    write_out("out_ext_n.bin", &n_ranges, 8);
    write_out("out_ext_runs.bin", runs, lines * 4);
    write_out("out_ext_allow.bin", allow, lines * 8);
    write_out("out_ext_hist.bin", hist, hw * 8);
    write_out("out_ext_k.bin", &k, 4);
    cls_engine_destroy(e);
    printf("reachext: %u endpoints (af %d), %u probes, %u ACLs, %u address classes, %llu ranges\n", n, v16 ? 16 : 4, p,
           n_acls, k, (unsigned long long)n_ranges);
    return 0;
}
