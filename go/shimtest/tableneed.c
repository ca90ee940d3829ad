/*
 * tableneed -- the Go binding's necessity-sweep shim (clsg_table_need,
 * include/contivcls_go.h) driven from plain C the way
 * go/contivcls/contivcls.go's TableNeed drives it;
 * tests/test_gpu_table_need.py checks its outputs against the reference.
 *
 * usage: tableneed DIR [SKIP]
 *   DIR/acls.txt   as reachtest's; the first ACL is swept
 *   SKIP           one rule treated as deleted
 * writes DIR/out_need_need.bin and out_need_free.bin (r u8 each),
 * out_need_first.bin (r + 1 u64), out_need_changed.bin (r u64),
 * out_need_witness.bin (r 16-byte records), out_need_counts.bin (4 u32),
 * out_need_n.bin (u64: the cells) and out_need_dims.bin (4 u32).
 */
#define _POSIX_C_SOURCE 200809L   /* strdup */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "contivcls_go.h"

static char dir[4096];

static void die(const char* what, cls_engine* e, int rc) {
    fprintf(stderr, "tableneed: %s failed (rc %d): %s\n", what, rc, e ? cls_last_error(e) : "");
    exit(1);
}

static FILE* open_in(const char* name, const char* mode) {
    char p[4200];
    snprintf(p, sizeof p, "%s/%s", dir, name);
    FILE* f = fopen(p, mode);
    if (!f) {
        fprintf(stderr, "tableneed: cannot open %s\n", p);
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

int main(int argc, char** argv) {
    if (argc != 2 && argc != 3) {
        fprintf(stderr, "usage: tableneed DIR [SKIP]\n");
        return 2;
    }
    snprintf(dir, sizeof dir, "%s", argv[1]);
    if (cls_abi_version() != clsg_abi_version()) {
        fprintf(stderr, "tableneed: library ABI %d, shims %d\n", cls_abi_version(), clsg_abi_version());
        return 1;
    }
    int devs[1] = {0};
    cls_engine* e = NULL;
    int rc = clsg_engine_create(devs, 1, &e);
    if (rc != CLS_OK) die("clsg_engine_create", NULL, rc);

    /* ---- ACLs, installed as they are read --------------------------------- */
    uint32_t n_acls = 0;
    char first_acl[128] = "";
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
        if (n_acls++ == 0) snprintf(first_acl, sizeof first_acl, "%s", name);
    }
    fclose(f);
    if (n_acls == 0) return 1;

    /* ---- the sweep of the first ACL's table through the shim ---------------- */
    uint32_t id = 0;
    cls_table_info info;
    if ((rc = cls_acl_table(e, first_acl, &id)) != CLS_OK) die("cls_acl_table", e, rc);
    if ((rc = cls_table_get_info(e, id, &info)) != CLS_OK) die("cls_table_get_info", e, rc);
    const size_t r = info.n_rules;
    uint64_t* skip = calloc((r + 63) / 64 + 1, 8);
    if (argc == 3) {
        const unsigned long k = strtoul(argv[2], NULL, 10);
        if (k >= r) return 2;
        skip[k >> 6] |= 1ull << (k & 63);
    }
    uint8_t* need = malloc(r + 1);
    uint8_t* fre = malloc(r + 1);
    uint8_t* need2 = malloc(r + 1);
    uint64_t* first = malloc((r + 2) * 8);
    uint64_t* changed = malloc((r + 1) * 8);
    cls_need_witness* wit = malloc((r + 1) * sizeof(cls_need_witness));
    uint32_t counts[4] = {9, 9, 9, 9}, dims[4] = {0, 0, 0, 0}, dims2[4] = {0, 0, 0, 0};
    uint64_t n_cells = 0, n_cells2 = 0, sum = 0;
    memset(need, 0xEE, r + 1);
    memset(fre, 0xEE, r + 1);
    memset(need2, 0xEE, r + 1);
    memset(first, 0xEE, (r + 2) * 8);
    memset(changed, 0xEE, (r + 1) * 8);
    memset(wit, 0xEE, (r + 1) * sizeof(cls_need_witness));
    /* the need bytes alone: no second pass */
    if ((rc = clsg_table_need(e, id, skip, need2, NULL, NULL, NULL, NULL, NULL, &n_cells2, dims2, 0)) != CLS_OK)
        die("clsg_table_need", e, rc);
    /* the Go binding's call and the remaining outputs */
    if ((rc = clsg_table_need(e, id, skip, need, fre, first, changed, wit, counts, &n_cells, dims, 0)) != CLS_OK)
        die("clsg_table_need", e, rc);
    /* the element past each array stays as it was */
    const unsigned char* past = (const unsigned char*)&wit[r];
    for (size_t i = 0; i < sizeof(cls_need_witness); ++i)
        if (past[i] != 0xEE) return 1;
    if (need[r] != 0xEE || fre[r] != 0xEE || need2[r] != 0xEE || first[r + 1] != 0xEEEEEEEEEEEEEEEEull ||
        changed[r] != 0xEEEEEEEEEEEEEEEEull)
        return 1;
    uint32_t tally[4] = {0, 0, 0, 0};
    for (size_t k = 0; k <= r; ++k) sum += first[k];
    for (size_t k = 0; k < r; ++k) {
        if (need[k] > 3) return 1;
        ++tally[need[k]];
        if ((need[k] == CLS_NEED_NEEDED) != (wit[k].after != 0) || (need[k] == CLS_NEED_NEEDED) != (changed[k] != 0) ||
            (need[k] >= CLS_NEED_REDUNDANT) != (first[k] != 0) || (fre[k] && need[k] == CLS_NEED_NEEDED) ||
            (need[k] == CLS_NEED_DEAD && !fre[k]))
            return 1;
    }
    if (sum != n_cells || memcmp(tally, counts, sizeof tally) != 0 || n_cells2 != n_cells ||
        memcmp(dims, dims2, sizeof dims) != 0 || memcmp(need, need2, r) != 0 ||
        n_cells != (uint64_t)dims[0] * dims[1] * ((uint64_t)dims[2] + dims[3] + 2)) {
        fprintf(stderr, "tableneed: the outputs disagree with each other\n");
        return 1;
    }
    /* a sweep without an output, of an unknown table or with another flag is refused */
    if (clsg_table_need(e, id, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &n_cells2, dims2, 0) != CLS_E_INVAL ||
        clsg_table_need(e, id + 1000, NULL, need2, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0) != CLS_E_NOTFOUND ||
        clsg_table_need(e, id, NULL, need2, NULL, NULL, NULL, NULL, NULL, NULL, NULL, CLS_F_FORCE_LINEAR) !=
            CLS_E_INVAL) {
        fprintf(stderr, "tableneed: a malformed sweep was accepted\n");
        return 1;
    }
    write_out("out_need_need.bin", need, r);
    write_out("out_need_free.bin", fre, r);
    write_out("out_need_first.bin", first, (r + 1) * 8);
    write_out("out_need_changed.bin", changed, r * 8);
    write_out("out_need_witness.bin", wit, r * sizeof(cls_need_witness));
    write_out("out_need_counts.bin", counts, sizeof counts);
    write_out("out_need_n.bin", &n_cells, 8);
    write_out("out_need_dims.bin", dims, sizeof dims);
    cls_engine_destroy(e);
    printf("tableneed: ACL %s, %zu rules, %llu cells, %u dead, %u redundant, %u needed\n", first_acl, r,
           (unsigned long long)n_cells, counts[CLS_NEED_DEAD], counts[CLS_NEED_REDUNDANT], counts[CLS_NEED_NEEDED]);
    return 0;
}
