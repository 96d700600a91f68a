/*
 * lpm_live_replay.c — stand-alone replay of a mutation stream on the host
 * LPM table (lpm_build.c + lpm_live.c), meant to be built with
 * -fsanitize=address,undefined (tests/test_lpm_live.py does so).
 *
 * Input file: "max_rules number_tbl8s n_rules n_ops", then n_rules lines
 * "ip depth next_hop" (the table cop_lpm_build starts from), then n_ops lines
 * "A ip depth next_hop" or "D ip depth 0". Every 100 operations the table's
 * interval export, its rule-id lookup and a DIR-24-8 image kept current by
 * patch records are compared with a brute-force longest-prefix match over the
 * rules the table exports.
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cop_internal.h"

#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
            exit(1);                                                 \
        }                                                            \
    } while (0)

static uint32_t mask_of(uint32_t depth) { return depth ? (uint32_t)(0xFFFFFFFFull << (32 - depth)) : 0u; }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

/* index into rules of the longest match, -1 on a miss */
static int brute(const cop_prefix *r, int n, uint32_t ip)
{
    int best = -1;
    for (int i = 0; i < n; i++)
        if ((ip & mask_of(r[i].depth)) == r[i].ip && (best < 0 || r[i].depth > r[best].depth)) best = i;
    return best;
}

static void check(const cop_lpm_table *t, cop_live_img *img, uint32_t *t24, uint32_t *t8, uint32_t cap8)
{
    const int n = cop_lpm_export_rules(t, NULL, 0);
    CHECK(n >= 0);
    cop_prefix *r = (cop_prefix *)malloc(sizeof(cop_prefix) * (size_t)(n ? n : 1));
    uint32_t *ids = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(n ? n : 1));
    CHECK(r && ids);
    CHECK(cop_lpm_export_rules_ids(t, r, ids, (uint32_t)n) == n);
    const int m = cop_lpm_export_intervals(t, NULL, NULL, 0xFFFFFFFFu);
    CHECK(m >= 1);
    uint32_t *s = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)m), *v = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)m);
    CHECK(s && v && cop_lpm_export_intervals(t, s, v, (uint32_t)m) == m);
    CHECK(s[0] == 0);
    for (int k = 1; k < m; k++) CHECK(s[k] > s[k - 1] && v[k] != v[k - 1]);
    /* the image follows the table by patch records */
    cop_patch_rec *recs = NULL;
    uint32_t n_recs = 0;
    cop_update_report rep;
    const int prc = cop_lpm_patch_records(t, img, &recs, &n_recs, &rep);
    if (prc) fprintf(stderr, "cop_lpm_patch_records: %d\n", prc);
    CHECK(prc == 0);
    CHECK(cop_patch_apply_host(t24, 1u << 24, t8, cap8, recs, n_recs) == 0);
    free(recs);
    CHECK(cop_live_img_generation(img) == cop_lpm_generation(t));
    for (int q = 0; q < 600; q++) {
        /* half the probes on a rule's edges */
        uint32_t ip = rnd();
        if (n && (q & 1)) {
            const cop_prefix *p = &r[rnd() % (uint32_t)n];
            const uint32_t lo = p->ip, hi = p->ip | ~mask_of(p->depth);
            const uint32_t pick[6] = {lo - 1, lo, lo + 1, hi - 1, hi, hi + 1};
            ip = pick[rnd() % 6];
        }
        const int b = brute(r, n, ip);
        const uint32_t want = b < 0 ? 0u : (r[b].next_hop | 0x01000000u);
        int lo = 0, hi = m;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (s[mid] <= ip) lo = mid;
            else hi = mid;
        }
        CHECK(v[lo] == want);
        int32_t rid = 0;
        CHECK(cop_lpm_lookup_rules(t, &ip, 1, &rid) == 0);
        CHECK(rid == (b < 0 ? -1 : (int32_t)ids[b]));
        uint32_t e = t24[ip >> 8];
        if ((e & COP_DIR_VALID_EXT) == COP_DIR_VALID_EXT) {
            CHECK((e & 0x00FFFFFFu) * 256u + 255u < cap8);
            e = t8[(e & 0x00FFFFFFu) * 256u + (ip & 0xFFu)];
        }
        CHECK((e & COP_IV_NHHIT) == want);
        uint32_t nh = 0;
        if (b >= 0) CHECK(cop_lpm_is_rule_present(t, r[b].ip, r[b].depth, &nh) == 1 && nh == r[b].next_hop);
    }
    free(r);
    free(ids);
    free(s);
    free(v);
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    CHECK(f);
    unsigned max_rules, tbl8s, n_rules, n_ops;
    CHECK(fscanf(f, "%u %u %u %u", &max_rules, &tbl8s, &n_rules, &n_ops) == 4);
    cop_prefix *rules = (cop_prefix *)calloc(n_rules ? n_rules : 1, sizeof(cop_prefix));
    CHECK(rules);
    for (unsigned i = 0; i < n_rules; i++) {
        unsigned ip, depth, nh;
        CHECK(fscanf(f, "%u %u %u", &ip, &depth, &nh) == 3);
        rules[i].ip = ip;
        rules[i].depth = (uint8_t)depth;
        rules[i].next_hop = nh;
    }
    cop_lpm_config cfg = {max_rules, tbl8s, 0};
    cop_lpm_table *t = NULL;
    CHECK(cop_lpm_build(rules, n_rules, &cfg, &t, NULL) == 0);
    free(rules);

    /* twice the table's groups: within one update a /24 early in the address
     * space may take a group before a later /24 gives its own back */
    const uint32_t cap_groups = 2 * tbl8s;
    uint32_t *t24 = (uint32_t *)malloc(sizeof(uint32_t) << 24);
    uint32_t *t8 = (uint32_t *)calloc((size_t)cap_groups * 256, sizeof(uint32_t));
    CHECK(t24 && t8);
    CHECK(cop_lpm_form_n_ext(t, COP_FORM_NH) <= cap_groups);
    cop_lpm_form_fill_dir24(t, COP_FORM_NH, t24, t8);
    cop_live_img *img = cop_live_img_create(t, COP_FORM_NH, cap_groups);
    CHECK(img);
    check(t, img, t24, t8, cap_groups * 256);

    unsigned done = 0, failed = 0;
    for (unsigned i = 0; i < n_ops; i++) {
        char op;
        unsigned ip, depth, nh;
        CHECK(fscanf(f, " %c %u %u %u", &op, &ip, &depth, &nh) == 4);
        const uint64_t g = cop_lpm_generation(t);
        const int rc = op == 'A' ? cop_lpm_add(t, ip, (uint8_t)depth, nh) : cop_lpm_delete(t, ip, (uint8_t)depth);
        CHECK(rc == 0 || rc == -ENOSPC || rc == -EINVAL);
        CHECK(cop_lpm_generation(t) == g + (rc == 0));
        failed += rc != 0;
        done++;
        if (done % 100 == 0) check(t, img, t24, t8, cap_groups * 256);
    }
    fclose(f);
    printf("replayed %u mutations (%u refused)\n", done, failed);
    printf("held %d generation %llu\n", cop_lpm_export_rules(t, NULL, 0), (unsigned long long)cop_lpm_generation(t));

    /* delete_all, an empty table's edges, and a table made by cop_lpm_create */
    CHECK(cop_lpm_delete_all(t) == 0);
    check(t, img, t24, t8, cap_groups * 256);
    CHECK(cop_lpm_add(t, 0, 1, 7) == 0 && cop_lpm_add(t, 0xFFFFFFFFu, 32, 8) == 0 && cop_lpm_add(t, 0, 32, 9) == 0);
    check(t, img, t24, t8, cap_groups * 256);
    CHECK(cop_lpm_delete(t, 0, 1) == 0 && cop_lpm_delete(t, 0, 1) == -EINVAL);
    check(t, img, t24, t8, cap_groups * 256);
    cop_lpm_table *e = NULL;
    CHECK(cop_lpm_create(NULL, &e) == 0);
    CHECK(cop_lpm_is_rule_present(e, 0, 8, NULL) == 0 && cop_lpm_delete(e, 0, 8) == -EINVAL);
    CHECK(cop_lpm_journal_set_cap(e, 4) == 0);
    for (uint32_t i = 0; i < 10; i++) CHECK(cop_lpm_add(e, i << 24, 8, i) == 0);
    cop_lpm_change *chg = NULL;
    CHECK(cop_lpm_changes_since(e, 0, &chg) == -ESTALE && chg == NULL);
    CHECK(cop_lpm_changes_since(e, 6, &chg) == 4 && chg[3].ip == 9u << 24 && chg[0].kind == COP_CHG_ADD);
    free(chg);
    cop_lpm_free(e);
    cop_live_img_free(img);
    cop_lpm_free(t);
    free(t24);
    free(t8);
    return 0;
}
