/*
 * reachclasses -- the Go binding's reachability-classes shims
 * (clsg_reach_classes_v4 / clsg_reach_classes_v16, include/contivcls_go.h)
 * driven from plain C the way go/contivcls/contivcls.go's ReachClasses drives
 * them; tests/test_gpu_reach_classes.py checks its outputs against the Python
 * call's.
 *
 * usage: reachclasses DIR 4|16
 *   DIR/acls.txt, DIR/ifs.txt, DIR/reach.bin   as reachtest's
 * writes DIR/out_classes.bin (n u32), DIR/out_classes_n.bin (C and the rounds
 * taken, u32 each), DIR/out_classes_rep.bin and DIR/out_classes_size.bin (C
 * u32 each), DIR/out_classes_self.bin (p x C bytes), DIR/out_classes_quot.bin
 * (p x C x C bytes) and DIR/out_classes_verdict.bin (p x n x n bytes).
 */
#define _POSIX_C_SOURCE 200809L   /* strdup */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "contivcls_go.h"

#define MAX_IFS 1024

static char dir[4096];

static void die(const char* what, cls_engine* e, int rc) {
    fprintf(stderr, "reachclasses: %s failed (rc %d): %s\n", what, rc, e ? cls_last_error(e) : "");
    exit(1);
}

static FILE* open_in(const char* name, const char* mode) {
    char p[4200];
    snprintf(p, sizeof p, "%s/%s", dir, name);
    FILE* f = fopen(p, mode);
    if (!f) {
        fprintf(stderr, "reachclasses: cannot open %s\n", p);
        exit(1);
    }
    return f;
}

static void* read_n(FILE* f, size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    if (!p || (bytes && fread(p, 1, bytes, f) != bytes)) {
        fprintf(stderr, "reachclasses: short input\n");
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
        fprintf(stderr, "usage: reachclasses DIR 4|16\n");
        return 2;
    }
    const int v16 = strcmp(argv[2], "16") == 0;
    snprintf(dir, sizeof dir, "%s", argv[1]);
    if (cls_abi_version() != clsg_abi_version()) {
        fprintf(stderr, "reachclasses: library ABI %d, shims %d\n", cls_abi_version(), clsg_abi_version());
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


    /* ---- the classes: endpoints and probes through the shims ------------------ */
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
    if (p < 1 || n < 1) return 1;
    const size_t cells = (size_t)p * n * n;
    uint32_t* classes = malloc((size_t)n * 4);
    uint8_t* verdict = malloc(cells);
    uint32_t count[2] = {0, 0};                 /* C, rounds */
    memset(classes, 0xEE, (size_t)n * 4);
    memset(verdict, 0xEE, cells);
    /* as the binding: room for two classes first, then for all of them */
    uint64_t cap = 2;
    uint32_t *rep = NULL, *size = NULL;
    uint8_t *self = NULL, *quot = NULL;
    for (int turn = 0; turn < 2; ++turn) {
        rep = malloc((size_t)cap * 4);
        size = malloc((size_t)cap * 4);
        self = malloc((size_t)p * cap);
        quot = malloc((size_t)p * cap * cap);
        memset(rep, 0xEE, (size_t)cap * 4);
        memset(quot, 0xEE, (size_t)p * cap * cap);
        rc = v16 ? clsg_reach_classes_v16(e, ifs, addr, n, proto, sport, dport, p, classes, &count[0], cap, rep, size,
                                          self, quot, verdict, &count[1], 0)
                 : clsg_reach_classes_v4(e, ifs, addr, n, proto, sport, dport, p, classes, &count[0], cap, rep, size,
                                         self, quot, verdict, &count[1], 0);
        if (rc != CLS_OK) die("clsg_reach_classes", e, rc);
        if (count[0] <= cap) break;
        /* too many classes for the room: the per-class outputs were left alone */
        if (turn == 1 || rep[0] != 0xEEEEEEEEu || quot[0] != 0xEE) {
            fprintf(stderr, "reachclasses: per-class outputs written past class_cap\n");
            return 1;
        }
        cap = count[0];
        free(rep);
        free(size);
        free(self);
        free(quot);
    }
    /* classes without class_out and n_classes, or per-class outputs without room, are refused and write nothing */
    const uint32_t was = classes[0];
    if (clsg_reach_classes_v4(e, ifs, addr, n, proto, sport, dport, p, NULL, NULL, cap, rep, size, self, quot, NULL, NULL,
                              0) != CLS_E_INVAL ||
        clsg_reach_classes_v4(e, ifs, addr, n, proto, sport, dport, p, classes, &count[0], 0, rep, NULL, NULL, NULL, NULL,
                              NULL, 0) != CLS_E_INVAL ||
        classes[0] != was) {
        fprintf(stderr, "reachclasses: a malformed call was accepted\n");
        return 1;
    }
    const size_t c = count[0];
    if (classes[0] != 0 || rep[0] != 0) return 1;
    write_out("out_classes.bin", classes, (size_t)n * 4);
    write_out("out_classes_n.bin", count, sizeof count);
    write_out("out_classes_rep.bin", rep, c * 4);
    write_out("out_classes_size.bin", size, c * 4);
    write_out("out_classes_self.bin", self, (size_t)p * c);
    write_out("out_classes_quot.bin", quot, (size_t)p * c * c);
    write_out("out_classes_verdict.bin", verdict, cells);
    cls_engine_destroy(e);
    printf("reachclasses: %u endpoints (af %d), %u probes, %u ACLs, %u classes in %u round(s)\n", n, v16 ? 16 : 4, p,
           n_acls, count[0], count[1]);
    return 0;
}
