/*
 * paint_plan_check.c — stand-alone check of the whole-image paint on the host
 * (lpm_build.c + lpm_live.c), meant to be built with
 * -fsanitize=address,undefined (tests/test_paint_plan.py does so).
 *
 * Input file: "max_rules number_tbl8s n_rules n_ops", then n_rules lines
 * "ip depth next_hop" (the table cop_lpm_build starts from), then n_ops lines
 * "A ip depth next_hop" or "D ip depth 0" (lpm_live_replay.c's format). For
 * both image forms, before and after the operations, cop_paint_host over
 * cop_lpm_paint_plan must equal cop_lpm_form_fill_dir24 word for word on a
 * tbl8 of n_ext + 3 groups, with the word after it untouched.
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

static int images = 0;

static void check(const cop_lpm_table *t, int form)
{
    uint32_t *s = NULL, *e = NULL, *x = NULL, niv = 0, n_ext = 0;
    CHECK(cop_lpm_paint_plan(t, form, &s, &e, &niv, &x, &n_ext) == 0);
    CHECK(niv >= 1 && s[0] == 0 && n_ext == cop_lpm_form_n_ext(t, form));
    for (uint32_t k = 1; k < niv; k++) CHECK(s[k] > s[k - 1]);
    for (uint32_t g = 0; g < n_ext; g++) CHECK(x[g] < (1u << 24) && (g == 0 || x[g] > x[g - 1]));
    const uint32_t cap = n_ext + 3;
    const size_t w8 = (size_t)cap * 256;
    uint32_t *a24 = (uint32_t *)malloc(sizeof(uint32_t) << 24), *b24 = (uint32_t *)malloc(sizeof(uint32_t) << 24);
    /* exactly cap groups and one guard word: a write past them is the sanitizer's to find */
    uint32_t *a8 = (uint32_t *)calloc(w8, sizeof(uint32_t)), *b8 = (uint32_t *)malloc((w8 + 1) * sizeof(uint32_t));
    CHECK(a24 && b24 && a8 && b8);
    memset(b24, 0xAB, sizeof(uint32_t) << 24);
    memset(b8, 0xAB, (w8 + 1) * sizeof(uint32_t));
    cop_lpm_form_fill_dir24(t, form, a24, a8);
    CHECK(cop_paint_host(s, e, niv, x, n_ext, b24, b8, cap) == 0);
    CHECK(memcmp(a24, b24, sizeof(uint32_t) << 24) == 0);
    CHECK(memcmp(a8, b8, w8 * sizeof(uint32_t)) == 0);
    CHECK(b8[w8] == 0xABABABABu);
    /* the launch guard */
    CHECK(cop_paint_host(s, e, 0, x, n_ext, b24, b8, cap) == -EINVAL);
    CHECK(cop_paint_host(s, e, niv, x, cap + 1, b24, b8, cap) == -EINVAL);
    if (niv > 1) CHECK(cop_paint_host(s + 1, e + 1, niv - 1, x, n_ext, b24, b8, cap) == -EINVAL);
    CHECK(memcmp(a24, b24, sizeof(uint32_t) << 24) == 0);
    free(a24);
    free(b24);
    free(a8);
    free(b8);
    free(s);
    free(e);
    free(x);
    images++;
}

int main(int argc, char **argv)
{
    CHECK(argc == 2);
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
    check(t, COP_FORM_NH);
    check(t, COP_FORM_RULE);
    for (unsigned i = 0; i < n_ops; i++) {
        char op;
        unsigned ip, depth, nh;
        CHECK(fscanf(f, " %c %u %u %u", &op, &ip, &depth, &nh) == 4);
        /* -ENOSPC / -EINVAL leave the table as it was: the stream may hold such steps */
        if (op == 'A') (void)cop_lpm_add(t, ip, (uint8_t)depth, nh);
        else (void)cop_lpm_delete(t, ip, (uint8_t)depth);
    }
    fclose(f);
    if (n_ops) {
        check(t, COP_FORM_NH);
        check(t, COP_FORM_RULE);
    }
    printf("painted %d images generation %llu\n", images, (unsigned long long)cop_lpm_generation(t));
    cop_lpm_free(t);
    return 0;
}
