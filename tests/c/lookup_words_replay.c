/*
 * lookup_words_replay.c — stand-alone check of the bulk-lookup host reference
 * (lpm_lookup.c: cop_lpm_lookup_words, cop_lpm_audit_probes) on a table under
 * live mutations (lpm_build.c + lpm_live.c), meant to be built with
 * -fsanitize=address,undefined (tests/test_lookup_words.py does so).
 *
 * Input file: lpm_live_replay.c's format: "max_rules number_tbl8s n_rules
 * n_ops", n_rules lines "ip depth next_hop", n_ops lines "A ip depth
 * next_hop" or "D ip depth 0". Before the first and after every 100th
 * operation both forms' words, over random addresses, rule edges and the
 * whole audit probe set, are compared with a brute-force longest-prefix match
 * over the rules the table exports, and the probe set with the intervals.
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

static uint32_t want_word(const cop_prefix *r, const uint32_t *ids, int n, int form, uint32_t ip)
{
    const int b = brute(r, n, ip);
    if (b < 0) return 0u;
    if (form == COP_LOOKUP_NH) return (r[b].next_hop & 0x00FFFFFFu) | COP_LOOKUP_HIT;
    return ids[b] | COP_LOOKUP_HIT | (r[b].next_hop ? COP_LOOKUP_DROP : 0u);
}

static unsigned long long n_words = 0, n_probe_words = 0;

static void check(const cop_lpm_table *t, int sample)
{
    const int n = cop_lpm_export_rules(t, NULL, 0);
    CHECK(n >= 0);
    cop_prefix *r = (cop_prefix *)malloc(sizeof(cop_prefix) * (size_t)(n ? n : 1));
    uint32_t *ids = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(n ? n : 1));
    CHECK(r && ids);
    CHECK(cop_lpm_export_rules_ids(t, r, ids, (uint32_t)n) == n);

    /* random addresses and rule edges, in one call per form */
    enum { Q = 600 };
    uint32_t ip[Q], w[Q];
    for (int q = 0; q < Q; q++) {
        ip[q] = rnd();
        if (n && (q & 1)) {
            const cop_prefix *p = &r[rnd() % (uint32_t)n];
            const uint32_t lo = p->ip, hi = p->ip | ~mask_of(p->depth);
            const uint32_t pick[6] = {lo - 1, lo, lo + 1, hi - 1, hi, hi + 1};
            ip[q] = pick[rnd() % 6];
        }
    }
    for (int form = COP_LOOKUP_NH; form <= COP_LOOKUP_RULE; form++) {
        memset(w, 0xEE, sizeof(w));
        CHECK(cop_lpm_lookup_words(t, form, ip, Q, w) == 0);
        for (int q = 0; q < Q; q++) {
            CHECK(w[q] == want_word(r, ids, n, form, ip[q]));
            CHECK((w[q] & ~(form == COP_LOOKUP_NH ? COP_LOOKUP_NH_MASK : COP_LOOKUP_RULE_MASK)) == 0);
        }
        n_words += Q;

        /* the audit's probe set against the form's intervals */
        uint32_t *s = NULL, *v = NULL;
        const uint32_t m = cop_lpm_form_intervals(t, form, &s, &v);
        CHECK(s && v && m >= 1 && s[0] == 0);
        uint32_t *pr = NULL, np = 0;
        CHECK(cop_lpm_audit_probes(t, form, &pr, &np) == 0);
        CHECK(pr && np >= 1 && np <= 2 * m + 1 && pr[0] == 0 && pr[np - 1] == 0xFFFFFFFFu);
        for (uint32_t i = 1; i < np; i++) CHECK(pr[i] > pr[i - 1]);
        uint32_t j = 0;   /* every start and the address before it are probes (both lists ascend) */
        for (uint32_t k = 0; k < m; k++) {
            if (s[k] > 0) {
                while (j < np && pr[j] < s[k] - 1u) j++;
                CHECK(j < np && pr[j] == s[k] - 1u);
            }
            while (j < np && pr[j] < s[k]) j++;
            CHECK(j < np && pr[j] == s[k]);
        }
        /* their words: all of them when the set is small, else a sample (the
         * brute force is O(rules) per address) */
        uint32_t *pw = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)np);
        CHECK(pw);
        CHECK(cop_lpm_lookup_words(t, form, pr, np, pw) == 0);
        const uint32_t step = sample && np > 2000 ? np / 1000 : 1;
        for (uint32_t i = 0; i < np; i += step) {
            CHECK(pw[i] == want_word(r, ids, n, form, pr[i]));
            n_probe_words++;
        }
        /* a probe pair straddles every boundary: in the merged next-hop form
         * the words on its two sides differ */
        for (uint32_t k = 1; k < m && form == COP_LOOKUP_NH; k++) CHECK(v[k] != v[k - 1]);
        free(pw);
        free(pr);
        free(s);
        free(v);
    }
    free(r);
    free(ids);
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

    /* refusals */
    uint32_t one = 1, w1 = 0xEEEEEEEEu;
    CHECK(cop_lpm_lookup_words(NULL, COP_LOOKUP_NH, &one, 1, &w1) == -EINVAL);
    CHECK(cop_lpm_lookup_words(t, 2, &one, 1, &w1) == -EINVAL && cop_lpm_lookup_words(t, -1, &one, 1, &w1) == -EINVAL);
    CHECK(cop_lpm_lookup_words(t, COP_LOOKUP_NH, NULL, 1, &w1) == -EINVAL);
    CHECK(cop_lpm_lookup_words(t, COP_LOOKUP_NH, &one, 1, NULL) == -EINVAL && w1 == 0xEEEEEEEEu);
    CHECK(cop_lpm_lookup_words(t, COP_LOOKUP_RULE, NULL, 0, NULL) == 0);
    uint32_t *pr = NULL, np = 0;
    CHECK(cop_lpm_audit_probes(NULL, COP_LOOKUP_NH, &pr, &np) == -EINVAL && cop_lpm_audit_probes(t, 7, &pr, &np) == -EINVAL);

    check(t, 1);
    unsigned done = 0, failed = 0;
    for (unsigned i = 0; i < n_ops; i++) {
        char op;
        unsigned ip, depth, nh;
        CHECK(fscanf(f, " %c %u %u %u", &op, &ip, &depth, &nh) == 4);
        const int rc = op == 'A' ? cop_lpm_add(t, ip, (uint8_t)depth, nh) : cop_lpm_delete(t, ip, (uint8_t)depth);
        CHECK(rc == 0 || rc == -ENOSPC || rc == -EINVAL);
        failed += rc != 0;
        done++;
        if (done % 100 == 0) check(t, 1);
    }
    fclose(f);
    printf("replayed %u mutations (%u refused)\n", done, failed);
    printf("held %d generation %llu\n", cop_lpm_export_rules(t, NULL, 0), (unsigned long long)cop_lpm_generation(t));

    /* the empty table, and the two ends of the address space as interval starts */
    CHECK(cop_lpm_delete_all(t) == 0);
    check(t, 0);
    CHECK(cop_lpm_audit_probes(t, COP_LOOKUP_NH, &pr, &np) == 0 && np == 2 && pr[0] == 0 && pr[1] == 0xFFFFFFFFu);
    free(pr);
    CHECK(cop_lpm_add(t, 0, 32, 9) == 0 && cop_lpm_add(t, 0xFFFFFFFFu, 32, 0) == 0 && cop_lpm_add(t, 0x80000000u, 1, 7) == 0);
    check(t, 0);
    CHECK(cop_lpm_audit_probes(t, COP_LOOKUP_RULE, &pr, &np) == 0);
    /* intervals [0], [1, 2^31 - 1], [2^31, 2^32 - 2], [2^32 - 1] */
    CHECK(np == 6 && pr[0] == 0 && pr[1] == 1 && pr[2] == 0x7FFFFFFFu && pr[3] == 0x80000000u && pr[4] == 0xFFFFFFFEu &&
          pr[5] == 0xFFFFFFFFu);
    free(pr);
    const uint32_t ends[2] = {0u, 0xFFFFFFFFu};
    uint32_t we[2];
    CHECK(cop_lpm_lookup_words(t, COP_LOOKUP_RULE, ends, 2, we) == 0);
    CHECK((we[0] & (COP_LOOKUP_HIT | COP_LOOKUP_DROP)) == (COP_LOOKUP_HIT | COP_LOOKUP_DROP));   /* action 9 */
    CHECK((we[1] & (COP_LOOKUP_HIT | COP_LOOKUP_DROP)) == COP_LOOKUP_HIT);                       /* action 0 */
    printf("words %llu probe words %llu\n", n_words, n_probe_words);
    cop_lpm_free(t);
    return 0;
}
