/*
 * acl_check.c — acl.c (cop_acl_build, cop_acl_match_host, cop_acl_*_host) over
 * exactly sized heap blocks. Built with -fsanitize=address,undefined by
 * tests/test_acl_host.py, so a byte read or written outside an extent stops
 * the program: every packet block ends 38 bytes past its last packet's start
 * (no byte past 37 is read), out_idx has exactly the list layout's capacity.
 * The values are checked against a linear scan of the rules written here and
 * against invariants of the specification (include/cop_gpu.h "ACL"): kept +
 * removed is the list's length, the counters sum to the entries that hit, an
 * entry is removed iff its word has COP_ACL_DROP.
 */
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cop_gpu.h"

#define CHECK(x)                                                           \
    do {                                                                   \
        if (!(x)) {                                                        \
            printf("acl_check: %s failed at line %d\n", #x, __LINE__);     \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static uint64_t rng_state = 0xACE1;
static uint32_t rnd(void)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static void *block(size_t bytes, size_t align)
{
    void *p = NULL;
    if (align < sizeof(void *)) align = sizeof(void *);
    CHECK(posix_memalign(&p, align, bytes ? bytes : 1) == 0);   /* ASan guards the exact size */
    return p;
}

static cop_acl_rule *make_rules(uint32_t n)
{
    static const uint8_t depths[] = {0, 1, 8, 16, 24, 31, 32};
    cop_acl_rule *r = block(sizeof(cop_acl_rule) * (size_t)n, 4);
    for (uint32_t i = 0; i < n; i++) {
        memset(&r[i], 0, sizeof(r[i]));
        r[i].src_ip = 0x0A000000u | (rnd() & 0xFFFF);
        r[i].dst_ip = rnd() & 1 ? 0xC0A80000u | (rnd() & 0xFF) : rnd() * 2u;
        r[i].src_depth = depths[rnd() % 7];
        r[i].dst_depth = depths[rnd() % 7];
        r[i].sport_lo = (uint16_t)(rnd() & 1 ? 0 : rnd());
        r[i].sport_hi = (uint16_t)(rnd() & 1 ? 0xFFFF : r[i].sport_lo + rnd() % (0x10000u - r[i].sport_lo));
        r[i].dport_lo = (uint16_t)(rnd() % 3 ? 0 : rnd());
        r[i].dport_hi = (uint16_t)(rnd() % 3 ? 0xFFFF : r[i].dport_lo);
        r[i].proto = (uint8_t)(rnd() & 1 ? 6 : 17);
        r[i].proto_mask = (uint8_t)(rnd() % 3 == 0 ? 0xFF : rnd() % 3 == 0 ? 0xF0 : 0);
        r[i].priority = (int32_t)(rnd() % 5) - 2;
        r[i].action = rnd() & 1;
    }
    return r;
}

static int rule_matches(const cop_acl_rule *r, const cop_acl_key *k)
{
    const uint32_t sm = r->src_depth ? 0xFFFFFFFFu << (32 - r->src_depth) : 0;
    const uint32_t dm = r->dst_depth ? 0xFFFFFFFFu << (32 - r->dst_depth) : 0;
    return ((k->src ^ r->src_ip) & sm) == 0 && ((k->dst ^ r->dst_ip) & dm) == 0 &&
           ((k->proto ^ r->proto) & r->proto_mask) == 0 && k->sport >= r->sport_lo && k->sport <= r->sport_hi &&
           k->dport >= r->dport_lo && k->dport <= r->dport_hi;
}

static uint32_t scan(const cop_acl_rule *r, uint32_t n, const cop_acl_key *k)
{
    int best = -1;
    for (uint32_t i = 0; i < n; i++)
        if (rule_matches(&r[i], k) && (best < 0 || r[i].priority > r[best].priority)) best = (int)i;
    return best < 0 ? 0 : (uint32_t)best | COP_ACL_HIT | (r[best].action ? COP_ACL_DROP : 0);
}

static cop_acl_key random_key(const cop_acl_rule *r, uint32_t n)
{
    cop_acl_key k;
    memset(&k, 0, sizeof(k));
    k.src = 0x0A000000u | (rnd() & 0xFFFF);
    k.dst = rnd() & 1 ? 0xC0A80000u | (rnd() & 0xFF) : rnd() * 2u;
    k.sport = (uint16_t)rnd();
    k.dport = (uint16_t)rnd();
    k.proto = (uint8_t)(rnd() & 1 ? 6 : rnd());
    if (n && rnd() % 4 == 0) {   /* on a rule's edges */
        const cop_acl_rule *x = &r[rnd() % n];
        k.src = x->src_ip, k.dst = x->dst_ip;
        k.sport = (uint16_t)(rnd() & 1 ? x->sport_lo : x->sport_hi + (rnd() & 1));
        k.dport = (uint16_t)(rnd() & 1 ? x->dport_hi : x->dport_lo - (rnd() & 1));
    }
    return k;
}

typedef struct {
    cop_batch b;
    cop_acl_desc d;
    uint32_t *want;   /* the word of every packet */
    uint32_t lists, count_words, idx_words;
} batch;

static batch make(const cop_acl_rule *r, uint32_t nr, uint32_t n, int imix, uint32_t stride, uint32_t data_off,
                  uint32_t n_lists, int seg)
{
    batch t;
    memset(&t, 0, sizeof(t));
    const uint32_t m = n ? n : 1;
    uint32_t *offsets = NULL;
    if (imix) {
        offsets = block(4 * (size_t)m, 4);
        for (uint32_t i = 0; i < m; i++) offsets[i] = (m - 1 - i) * 64;
        stride = 64;
    }
    const size_t bytes = (size_t)(m - 1) * stride + data_off + 38;   /* the last packet's bytes 0..37 and no more */
    uint8_t *pk = block(bytes, 16);
    for (size_t i = 0; i < bytes; i++) pk[i] = (uint8_t)rnd();
    t.want = block(4 * (size_t)m, 4);
    for (uint32_t i = 0; i < n; i++) {
        uint8_t *p = pk + (offsets ? offsets[i] : (size_t)i * stride) + data_off;
        const uint32_t kind = rnd() % 12;
        cop_acl_key k = random_key(r, nr);
        p[12] = kind == 0 ? 0x86 : 0x08, p[13] = kind == 0 ? 0xDD : 0x00;
        p[14] = kind == 1 ? 0x65 : kind == 2 ? 0x44 : kind == 3 ? 0x46 : 0x45;
        p[20] = (uint8_t)((p[20] & 0xC0) | (kind == 4 ? 0x20 : 0)), p[21] = kind == 5;
        p[23] = k.proto;
        p[26] = (uint8_t)(k.src >> 24), p[27] = (uint8_t)(k.src >> 16), p[28] = (uint8_t)(k.src >> 8), p[29] = (uint8_t)k.src;
        p[30] = (uint8_t)(k.dst >> 24), p[31] = (uint8_t)(k.dst >> 16), p[32] = (uint8_t)(k.dst >> 8), p[33] = (uint8_t)k.dst;
        p[34] = (uint8_t)(k.sport >> 8), p[35] = (uint8_t)k.sport, p[36] = (uint8_t)(k.dport >> 8), p[37] = (uint8_t)k.dport;
        if (kind == 3 || kind == 5) k.sport = k.dport = 0;
        t.want[i] = kind <= 2 ? COP_ACL_SKIP : scan(r, nr, &k);
    }
    t.b.pkts = pk;
    t.b.offsets = offsets;
    t.b.n = n;
    t.b.stride = imix ? 0 : stride;
    t.b.data_off = data_off;
    t.lists = n_lists;
    t.count_words = seg ? (n + COP_SEG_PKTS - 1) / COP_SEG_PKTS : n_lists;
    t.idx_words = n * (seg ? 1 : n_lists);
    t.b.fwd_idx = block(4 * (size_t)t.idx_words, 4);
    t.b.fwd_count = block(4 * (size_t)(t.count_words ? t.count_words : 1), 4);
    for (uint32_t i = 0; i < t.idx_words; i++) t.b.fwd_idx[i] = rnd() % (n + n / 8 + 1);   /* some indices >= n */
    for (uint32_t i = 0; i < t.count_words; i++) {
        const uint32_t cap = seg ? COP_SEG_PKTS : n;
        t.b.fwd_count[i] = rnd() % 4 == 0 ? 0xFFFFFFF0u : rnd() % (cap + 1);                  /* some above capacity */
    }
    t.d.words = block(4 * (size_t)n, 4);
    t.d.out_idx = block(4 * (size_t)t.idx_words, 4);
    t.d.out_count = block(4 * (size_t)(t.count_words ? t.count_words : 1), 4);
    t.d.status = block(16 * (size_t)n_lists, 16);
    return t;
}

static void drop(batch *t)
{
    free((void *)t->b.pkts), free((void *)t->b.offsets), free(t->b.fwd_idx), free(t->b.fwd_count), free(t->want);
    free(t->d.words), free(t->d.out_idx), free(t->d.out_count), free(t->d.status);
}

static uint32_t word_at(const batch *t, uint32_t e) { return t->want[e < t->b.n ? e : t->b.n - 1]; }

static void run(const cop_acl_rule *r, uint32_t nr, const cop_acl_table *tab, uint32_t n, int imix, uint32_t stride,
                uint32_t data_off, uint32_t n_lists, int seg)
{
    batch t[2] = {make(r, nr, n, imix, stride, data_off, n_lists, seg), make(r, nr, n / 2, imix, stride, 0, n_lists, seg)};
    cop_batch bs[2] = {t[0].b, t[1].b};
    cop_acl_desc ds[2] = {t[0].d, t[1].d};
    CHECK(cop_acl_classify_host(tab, bs, ds, 2, 0) == 0);
    uint64_t *ctr = block(8 * (size_t)nr, 8), hits = 0, counted = 0;
    memset(ctr, 0, 8 * (size_t)nr);
    CHECK(cop_acl_filter_host(tab, ctr, bs, ds, 2, n_lists, seg, 0) == 0);
    for (int j = 0; j < 2; j++) {
        const batch *x = &t[j];
        const uint32_t nn = x->b.n;
        for (uint32_t i = 0; i < nn; i++) CHECK(x->d.words[i] == x->want[i]);
        if (!nn) continue;
        uint32_t st[4] = {0, 0, 0, 0};
        for (uint32_t c = 0; c < x->count_words; c++) {
            const uint32_t cap = seg ? (nn - c * COP_SEG_PKTS < COP_SEG_PKTS ? nn - c * COP_SEG_PKTS : COP_SEG_PKTS) : nn;
            const uint32_t cnt = x->b.fwd_count[c] < cap ? x->b.fwd_count[c] : cap;
            const uint32_t *in = x->b.fwd_idx + (size_t)c * (seg ? COP_SEG_PKTS : nn);
            const uint32_t *out = x->d.out_idx + (size_t)c * (seg ? COP_SEG_PKTS : nn);
            uint32_t kept = 0, miss = 0, skip = 0;
            for (uint32_t k = 0; k < cnt; k++) {
                const uint32_t w = word_at(x, in[k]);
                hits += (w & COP_ACL_HIT) != 0;
                if (w & COP_ACL_DROP) continue;
                CHECK(out[kept] == in[k]);
                kept++, miss += w == 0, skip += w == COP_ACL_SKIP;
            }
            CHECK(x->d.out_count[c] == kept);
            if (!seg) {
                CHECK(x->d.status[4 * c] == kept && x->d.status[4 * c + 1] == cnt - kept);
                CHECK(x->d.status[4 * c + 2] == miss && x->d.status[4 * c + 3] == skip);
            } else {
                st[0] += kept, st[1] += cnt - kept, st[2] += miss, st[3] += skip;
            }
        }
        if (seg) CHECK(!memcmp(st, x->d.status, 16));
    }
    for (uint32_t i = 0; i < nr; i++) counted += ctr[i];
    CHECK(counted == hits);
    /* refused, and said so, before anything is touched: in place, and a stride of 32 */
    ds[0].out_idx = t[0].b.fwd_idx;
    if (n) CHECK(cop_acl_filter_host(tab, ctr, bs, ds, 2, n_lists, seg, 0) == -EINVAL);
    ds[0] = t[0].d;
    bs[0].stride = 32, bs[0].offsets = NULL;
    if (n) CHECK(cop_acl_classify_host(tab, bs, ds, 2, 0) == -EINVAL);
    free(ctr);
    drop(&t[0]), drop(&t[1]);
}

int main(void)
{
    static const uint32_t rule_counts[] = {0, 1, 33, 129, 1024};
    static const uint32_t ns[] = {0, 1, 255, 256, 257, 1027};
    for (size_t a = 0; a < sizeof(rule_counts) / sizeof(rule_counts[0]); a++) {
        const uint32_t nr = rule_counts[a];
        cop_acl_rule *r = make_rules(nr);
        cop_acl_table *tab = NULL;
        cop_acl_report rep;
        CHECK(cop_acl_build(r, nr, &tab, &rep) == 0 && tab);
        CHECK(rep.n_rules == nr && rep.row_words == 4 * (((nr ? nr : 1) + 127) / 128) && rep.first_error_idx == 0xFFFFFFFFu);
        for (int f = 0; f < 4; f++) CHECK(rep.n_intervals[f] >= 1 && rep.n_intervals[f] <= 2 * nr + 1);
        /* keys: exactly sized arrays */
        const uint32_t nk = 4096;
        cop_acl_key *keys = block(sizeof(cop_acl_key) * nk, 4);
        uint32_t *out = block(4 * nk, 4);
        for (uint32_t i = 0; i < nk; i++) keys[i] = random_key(r, nr);
        CHECK(cop_acl_match_host(tab, keys, nk, out) == 0);
        for (uint32_t i = 0; i < nk; i++) CHECK(out[i] == scan(r, nr, &keys[i]));
        free(keys), free(out);
        for (size_t b = 0; b < sizeof(ns) / sizeof(ns[0]); b++) {
            if (nr == 1024 && ns[b] != 1027 && ns[b] != 0) continue;
            run(r, nr, tab, ns[b], 0, 64, 0, 1, 0);
            run(r, nr, tab, ns[b], 0, 128, 16, 5, 0);
            run(r, nr, tab, ns[b], 1, 0, 16, 1, 1);
            run(r, nr, tab, ns[b], 0, 48, 0, 1, 1);
        }
        cop_acl_free(tab);
        /* a bad rule: nothing built */
        if (nr) {
            r[nr / 2].sport_lo = 9, r[nr / 2].sport_hi = 8;
            tab = (cop_acl_table *)r;
            CHECK(cop_acl_build(r, nr, &tab, &rep) == -EINVAL && tab == NULL && rep.first_error_idx == nr / 2);
            r[nr / 2].sport_hi = 9, r[nr / 2].dst_depth = 33;
            CHECK(cop_acl_build(r, nr, &tab, &rep) == -EINVAL && tab == NULL && rep.first_error_idx == nr / 2);
        }
        free(r);
    }
    cop_acl_table *tab = NULL;
    cop_acl_report rep;
    cop_acl_rule *big = make_rules(COP_ACL_MAX_RULES + 1);
    CHECK(cop_acl_build(big, COP_ACL_MAX_RULES + 1, &tab, &rep) == -ENOSPC && tab == NULL);
    free(big);
    cop_acl_free(NULL);
    printf("acl_check ok\n");
    return 0;
}
