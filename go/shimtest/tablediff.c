/*
 * tablediff -- the Go binding's table-diff shims (clsg_table_diff_v4 /
 * clsg_table_diff_v16, include/contivcls_go.h) driven from plain C the way
 * go/contivcls/contivcls.go's TableDiff drives them;
 * tests/test_gpu_table_diff.py checks its outputs against the reference.
 *
 * usage: tablediff DIR 4|16
 *   DIR/acls.txt   as reachtest's; the first ACL is diffed against the second
 * writes DIR/out_tdiff_n.bin (3 u64: n_diff, n_rec, the cells),
 * DIR/out_tdiff_pairs.bin (16 u64), DIR/out_tdiff_first.bin (one 16-byte
 * record), DIR/out_tdiff_cells_a.bin / _cells_b.bin (r + 1 u64),
 * DIR/out_tdiff_wit_a.bin / _wit_b.bin (r + 1 16-byte records),
 * DIR/out_tdiff_rec.bin (n_rec 32-byte records) and DIR/out_tdiff_dims.bin (4 u32).
 */
#define _POSIX_C_SOURCE 200809L   /* strdup */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "contivcls_go.h"

static char dir[4096];

static void die(const char* what, cls_engine* e, int rc) {
    fprintf(stderr, "tablediff: %s failed (rc %d): %s\n", what, rc, e ? cls_last_error(e) : "");
    exit(1);
}

static FILE* open_in(const char* name, const char* mode) {
    char p[4200];
    snprintf(p, sizeof p, "%s/%s", dir, name);
    FILE* f = fopen(p, mode);
    if (!f) {
        fprintf(stderr, "tablediff: cannot open %s\n", p);
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

typedef int (*diff_fn)(cls_engine*, uint32_t, uint32_t, uint64_t*, uint64_t*, void*, uint64_t*, void*, uint64_t*, void*,
                       void*, uint64_t, uint64_t*, uint64_t*, uint32_t*, uint32_t);

int main(int argc, char** argv) {
    if (argc != 3 || (strcmp(argv[2], "4") != 0 && strcmp(argv[2], "16") != 0)) {
        fprintf(stderr, "usage: tablediff DIR 4|16\n");
        return 2;
    }
    const int v16 = strcmp(argv[2], "16") == 0;
    snprintf(dir, sizeof dir, "%s", argv[1]);
    if (cls_abi_version() != clsg_abi_version()) {
        fprintf(stderr, "tablediff: library ABI %d, shims %d\n", cls_abi_version(), clsg_abi_version());
        return 1;
    }
    int devs[1] = {0};
    cls_engine* e = NULL;
    int rc = clsg_engine_create(devs, 1, &e);
    if (rc != CLS_OK) die("clsg_engine_create", NULL, rc);

    /* ---- ACLs, installed as they are read --------------------------------- */
    uint32_t n_acls = 0;
    char names[2][128] = {"", ""};
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
        if (n_acls < 2) snprintf(names[n_acls], sizeof names[0], "%s", name);
        ++n_acls;
    }
    fclose(f);
    if (n_acls < 2) return 1;

    /* ---- the diff of the first two ACLs' tables through the shims ------------- */
    uint32_t id[2] = {0, 0};
    size_t r[2] = {0, 0};
    for (int i = 0; i < 2; ++i) {
        cls_table_info info;
        if ((rc = cls_acl_table(e, names[i], &id[i])) != CLS_OK) die("cls_acl_table", e, rc);
        if ((rc = cls_table_get_info(e, id[i], &info)) != CLS_OK) die("cls_table_get_info", e, rc);
        r[i] = (size_t)info.n_rules + 1;
    }
    const diff_fn diff = v16 ? clsg_table_diff_v16 : clsg_table_diff_v4;
    /* the Go binding's first call: the record count alone */
    uint64_t n_rec = ~0ull, n_rec2 = ~0ull, n_diff = ~0ull, n_cells = 0, pairs[16], sum = 0;
    uint32_t dims[4] = {0, 0, 0, 0};
    if ((rc = diff(e, id[0], id[1], NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, &n_rec, NULL, NULL, 0)) != CLS_OK)
        die("clsg_table_diff (count)", e, rc);
    cls_cover_witness first;
    cls_cover_witness* wit[2];
    uint64_t* cells[2];
    for (int i = 0; i < 2; ++i) {
        wit[i] = malloc((r[i] + 1) * sizeof(cls_cover_witness));
        cells[i] = malloc((r[i] + 1) * 8);
        memset(wit[i], 0xEE, (r[i] + 1) * sizeof(cls_cover_witness));
        memset(cells[i], 0xEE, (r[i] + 1) * 8);
    }
    cls_tdiff_rec* rec = malloc((n_rec + 1) * sizeof(cls_tdiff_rec));
    memset(rec, 0xEE, (n_rec + 1) * sizeof(cls_tdiff_rec));
    if ((rc = diff(e, id[0], id[1], &n_diff, pairs, &first, cells[0], wit[0], cells[1], wit[1], rec, n_rec, &n_rec2,
                   &n_cells, dims, 0)) != CLS_OK)
        die("clsg_table_diff", e, rc);
    /* the element past each array stays as it was */
    const unsigned char* past = (const unsigned char*)&rec[n_rec];
    for (size_t i = 0; i < sizeof(cls_tdiff_rec); ++i)
        if (past[i] != 0xEE) return 1;
    for (int i = 0; i < 2; ++i) {
        past = (const unsigned char*)&wit[i][r[i]];
        for (size_t k = 0; k < sizeof(cls_cover_witness); ++k)
            if (past[k] != 0xEE) return 1;
        if (cells[i][r[i]] != 0xEEEEEEEEEEEEEEEEull) return 1;
        uint64_t side = 0;
        for (size_t k = 0; k < r[i]; ++k) {
            side += cells[i][k];
            if ((wit[i][k].live != 0) != (cells[i][k] != 0)) return 1;
        }
        if (side != n_diff) return 1;
    }
    for (int i = 0; i < 16; ++i) sum += pairs[i];
    for (uint64_t k = 0; k < n_rec; ++k)
        if (rec[k].was == rec[k].now || rec[k].zero) return 1;
    if (sum != n_cells || n_rec2 != n_rec || (n_diff != 0) != (first.live != 0) || (n_diff != 0) != (n_rec != 0) ||
        n_cells != (uint64_t)dims[0] * dims[1] * ((uint64_t)dims[2] + dims[3] + 2)) {
        fprintf(stderr, "tablediff: the outputs disagree with each other\n");
        return 1;
    }
    /* a table against itself: no difference */
    uint64_t self = ~0ull;
    if ((rc = diff(e, id[0], id[0], &self, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, 0)) != CLS_OK ||
        self != 0)
        die("clsg_table_diff (self)", e, rc);
    /* a diff without an output, of an unknown table, with a classify-only flag or records without a count is refused */
    if (diff(e, id[0], id[1], NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, &n_cells, dims, 0) != CLS_E_INVAL ||
        diff(e, id[0] + 1000, id[1], &self, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, 0) !=
            CLS_E_NOTFOUND ||
        diff(e, id[0], id[1], &self, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, CLS_F_TIMING) !=
            CLS_E_INVAL ||
        diff(e, id[0], id[1], NULL, NULL, NULL, NULL, NULL, NULL, NULL, rec, n_rec, NULL, NULL, NULL, 0) != CLS_E_INVAL) {
        fprintf(stderr, "tablediff: a malformed diff was accepted\n");
        return 1;
    }
    const uint64_t n[3] = {n_diff, n_rec, n_cells};
    write_out("out_tdiff_n.bin", n, sizeof n);
    write_out("out_tdiff_pairs.bin", pairs, sizeof pairs);
    write_out("out_tdiff_first.bin", &first, sizeof first);
    write_out("out_tdiff_cells_a.bin", cells[0], r[0] * 8);
    write_out("out_tdiff_cells_b.bin", cells[1], r[1] * 8);
    write_out("out_tdiff_wit_a.bin", wit[0], r[0] * sizeof(cls_cover_witness));
    write_out("out_tdiff_wit_b.bin", wit[1], r[1] * sizeof(cls_cover_witness));
    write_out("out_tdiff_rec.bin", rec, n_rec * sizeof(cls_tdiff_rec));
    write_out("out_tdiff_dims.bin", dims, sizeof dims);
    cls_engine_destroy(e);
    printf("tablediff: ACL %s against %s (af %d), %llu cells, %llu differ, %llu records\n", names[0], names[1],
           v16 ? 16 : 4, (unsigned long long)n_cells, (unsigned long long)n_diff, (unsigned long long)n_rec);
    return 0;
}
