/*
 * tablecover -- the Go binding's coverage-sweep shims (clsg_table_cover_v4 /
 * clsg_table_cover_v16, include/contivcls_go.h) driven from plain C the way
 * go/contivcls/contivcls.go's TableCover drives them;
 * tests/test_gpu_table_cover.py checks its outputs against the reference.
 *
 * usage: tablecover DIR 4|16
 *   DIR/acls.txt   as reachtest's; the first ACL is swept
 * writes DIR/out_cover_live.bin (r + 1 u8), DIR/out_cover_witness.bin (r + 1
 * 16-byte records), DIR/out_cover_cells.bin (r + 1 u64), DIR/out_cover_dead.bin
 * (u32), DIR/out_cover_n.bin (u64: the cells) and DIR/out_cover_dims.bin (4 u32).
 */
#define _POSIX_C_SOURCE 200809L   /* strdup */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "contivcls_go.h"

static char dir[4096];

static void die(const char* what, cls_engine* e, int rc) {
    fprintf(stderr, "tablecover: %s failed (rc %d): %s\n", what, rc, e ? cls_last_error(e) : "");
    exit(1);
}

static FILE* open_in(const char* name, const char* mode) {
    char p[4200];
    snprintf(p, sizeof p, "%s/%s", dir, name);
    FILE* f = fopen(p, mode);
    if (!f) {
        fprintf(stderr, "tablecover: cannot open %s\n", p);
        exit(1);
    }
    return f;
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

typedef int (*cover_fn)(cls_engine*, uint32_t, uint8_t*, void*, uint64_t*, uint32_t*, uint64_t*, uint32_t*, uint32_t);

int main(int argc, char** argv) {
    if (argc != 3 || (strcmp(argv[2], "4") != 0 && strcmp(argv[2], "16") != 0)) {
        fprintf(stderr, "usage: tablecover DIR 4|16\n");
        return 2;
    }
    const int v16 = strcmp(argv[2], "16") == 0;
    snprintf(dir, sizeof dir, "%s", argv[1]);
    if (cls_abi_version() != clsg_abi_version()) {
        fprintf(stderr, "tablecover: library ABI %d, shims %d\n", cls_abi_version(), clsg_abi_version());
        return 1;
    }
    int devs[1] = {0};
    cls_engine* e = NULL;
    int rc = clsg_engine_create(devs, 1, &e);
    if (rc != CLS_OK) die("clsg_engine_create", NULL, rc);

    /* ---- ACLs, installed as they are read --------------------------------- */
    uint32_t n_acls = 0;
    char first[128] = "";
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
        if (n_acls++ == 0) snprintf(first, sizeof first, "%s", name);
    }
    fclose(f);
    if (n_acls == 0) return 1;

    /* ---- the sweep of the first ACL's table through the shims --------------- */
    uint32_t id = 0;
    cls_table_info info;
    if ((rc = cls_acl_table(e, first, &id)) != CLS_OK) die("cls_acl_table", e, rc);
    if ((rc = cls_table_get_info(e, id, &info)) != CLS_OK) die("cls_table_get_info", e, rc);
    const size_t r = (size_t)info.n_rules + 1;
    const cover_fn cover = v16 ? clsg_table_cover_v16 : clsg_table_cover_v4;
    uint8_t* live = malloc(r + 1);
    cls_cover_witness* wit = malloc((r + 1) * sizeof(cls_cover_witness));
    uint64_t* cells = malloc((r + 1) * 8);
    uint32_t n_dead = ~0u, dims[4] = {0, 0, 0, 0}, dims2[4] = {0, 0, 0, 0};
    uint64_t n_cells = 0, n_cells2 = 0, sum = 0;
    memset(live, 0xEE, r + 1);
    memset(wit, 0xEE, (r + 1) * sizeof(cls_cover_witness));
    memset(cells, 0xEE, (r + 1) * 8);
    /* the Go binding's call: live bytes and witnesses alone */
    if ((rc = cover(e, id, live, wit, NULL, NULL, &n_cells2, dims2, 0)) != CLS_OK) die("clsg_table_cover", e, rc);
    uint8_t* live2 = malloc(r);
    memcpy(live2, live, r);
    if ((rc = cover(e, id, live, wit, cells, &n_dead, &n_cells, dims, 0)) != CLS_OK) die("clsg_table_cover", e, rc);
    /* the element past each array stays as it was */
    const unsigned char* past = (const unsigned char*)&wit[r];
    for (size_t i = 0; i < sizeof(cls_cover_witness); ++i)
        if (past[i] != 0xEE) return 1;
    if (live[r] != 0xEE || cells[r] != 0xEEEEEEEEEEEEEEEEull) return 1;
    uint32_t dead = 0;
    for (size_t k = 0; k < r; ++k) {
        sum += cells[k];
        if (k + 1 < r && !live[k]) ++dead;
        if (live[k] != wit[k].live || (live[k] != 0) != (cells[k] != 0)) return 1;
    }
    if (sum != n_cells || dead != n_dead || n_cells2 != n_cells || memcmp(dims, dims2, sizeof dims) != 0 ||
        memcmp(live, live2, r) != 0 ||
        n_cells != (uint64_t)dims[0] * dims[1] * ((uint64_t)dims[2] + dims[3] + 2)) {
        fprintf(stderr, "tablecover: the outputs disagree with each other\n");
        return 1;
    }
    /* a sweep without an output, of an unknown table or with a classify-only flag is refused */
    if (cover(e, id, NULL, NULL, NULL, NULL, &n_cells2, dims2, 0) != CLS_E_INVAL ||
        cover(e, id + 1000, live, NULL, NULL, NULL, NULL, NULL, 0) != CLS_E_NOTFOUND ||
        cover(e, id, live, NULL, NULL, NULL, NULL, NULL, CLS_F_TIMING) != CLS_E_INVAL) {
        fprintf(stderr, "tablecover: a malformed sweep was accepted\n");
        return 1;
    }
    write_out("out_cover_live.bin", live, r);
    write_out("out_cover_witness.bin", wit, r * sizeof(cls_cover_witness));
    write_out("out_cover_cells.bin", cells, r * 8);
    write_out("out_cover_dead.bin", &n_dead, 4);
    write_out("out_cover_n.bin", &n_cells, 8);
    write_out("out_cover_dims.bin", dims, sizeof dims);
    cls_engine_destroy(e);
    printf("tablecover: ACL %s (af %d), %zu rules, %llu cells, %u dead\n", first, v16 ? 16 : 4, r - 1,
           (unsigned long long)n_cells, n_dead);
    return 0;
}
