/*
 * sketch_check.c — sketch.c (cop_sketch_*_host) over exactly sized heap blocks.
 * Built with -fsanitize=address,undefined by tests/test_sketch_host.py, so a
 * byte read or written outside an extent stops the program; the values are
 * checked against invariants of the specification (include/cop_gpu.h "Sketch"):
 * every row's counters sum to the counting packets, an estimate is never below
 * the true count, kept + removed is the list's length, a threshold of 2^64 - 1
 * keeps everything, and nothing of out_idx is needed past the kept entries
 * (out_idx has exactly the list's capacity).
 */
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cop_gpu.h"

#define CHECK(x)                                                              \
    do {                                                                      \
        if (!(x)) {                                                           \
            printf("sketch_check: %s failed at line %d\n", #x, __LINE__);     \
            exit(1);                                                          \
        }                                                                     \
    } while (0)

static uint64_t rng_state = 0x1234;
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

typedef struct {
    cop_batch b;
    cop_police_desc p;
    uint32_t *keys;   /* the address of every packet */
    uint8_t *ipv4;
    uint32_t lists, count_words;
} batch;

/* layout: 0 slots of `stride` (data_off 0 or 128), 1 IMIX, 2 records */
static batch make(uint32_t n, int layout, uint32_t stride, uint32_t data_off, uint32_t n_lists, int seg, int dst)
{
    batch t;
    memset(&t, 0, sizeof(t));
    const uint32_t m = n ? n : 1;
    uint8_t *pk;
    uint32_t *offsets = NULL;
    size_t bytes;
    if (layout == 1) {
        offsets = block(4 * (size_t)m, 4);
        for (uint32_t i = 0; i < m; i++) offsets[i] = (m - 1 - i) * 64;
        bytes = (size_t)(m - 1) * 64 + data_off + 48;   /* the last packet's 48 readable bytes and no more */
        stride = 0;
    } else {
        if (layout == 2) stride = COP_HDR16_STRIDE;
        bytes = (size_t)(m - 1) * stride + data_off + (layout == 2 ? 16 : 48);
    }
    pk = block(bytes, 16);
    for (size_t i = 0; i < bytes; i++) pk[i] = (uint8_t)rnd();
    t.keys = block(4 * (size_t)m, 4);
    t.ipv4 = block(m, 1);
    cop_result *res = block(8 * (size_t)m, 8);
    for (uint32_t i = 0; i < n; i++) {
        uint8_t *p = pk + (offsets ? offsets[i] : (size_t)i * stride) + data_off;
        uint8_t *et = layout == 2 ? p : p + 12, *ad = layout == 2 ? p + 6 : p + 26;
        const uint32_t r = rnd() % 16;
        et[0] = r == 0 ? 0x86 : 0x08;
        et[1] = r == 0 ? 0xDD : 0x00;
        et[2] = r == 1 ? 0x65 : 0x45;
        t.ipv4[i] = r > 1;
        const uint32_t a = (rnd() & 1) ? 0x0A010203u : 0x0B000000u + rnd() % 4096;
        uint8_t *w = ad + (dst ? 4 : 0);
        w[0] = (uint8_t)(a >> 24), w[1] = (uint8_t)(a >> 16), w[2] = (uint8_t)(a >> 8), w[3] = (uint8_t)a;
        t.keys[i] = a;
        res[i].verdict = (uint8_t)(rnd() % 5);
    }
    t.b.pkts = pk;
    t.b.offsets = offsets;
    t.b.n = n;
    t.b.stride = stride;
    t.b.data_off = data_off;
    t.b.results = res;
    /* lists: every other packet, in the context's layout; counts above what the layout holds, an index >= n */
    t.lists = seg ? (n + COP_SEG_PKTS - 1) / COP_SEG_PKTS : n_lists;
    t.count_words = t.lists ? t.lists : 1;
    const size_t idx_words = (size_t)m * (seg ? 1 : n_lists);
    t.b.fwd_idx = block(4 * idx_words, 16);
    t.b.fwd_count = block(4 * (size_t)t.count_words, 4);
    t.p.out_idx = block(4 * idx_words, 16);
    t.p.out_count = block(4 * (size_t)t.count_words, 4);
    t.p.status = block(16 * (size_t)n_lists, 16);
    memset(t.p.out_idx, 0xAB, 4 * idx_words);
    for (size_t k = 0; k < idx_words; k++) t.b.fwd_idx[k] = (uint32_t)((2 * k) % m) + (k % 5 == 4 ? n : 0);
    for (uint32_t q = 0; q < t.count_words; q++) t.b.fwd_count[q] = q % 3 == 2 ? 0xFFFFFFFFu : (seg ? 100 + q : n / 2);
    return t;
}

static void drop(batch *t)
{
    free((void *)t->b.pkts);
    free((void *)t->b.offsets);
    free(t->b.results);
    free(t->b.fwd_idx);
    free(t->b.fwd_count);
    free(t->p.out_idx);
    free(t->p.out_count);
    free(t->p.status);
    free(t->keys);
    free(t->ipv4);
}

static uint32_t list_len(const batch *t, uint32_t q, int seg)
{
    const uint32_t n = t->b.n, c = t->b.fwd_count[q];
    if (!seg) return c < n ? c : n;
    const uint32_t cap = n - q * COP_SEG_PKTS < COP_SEG_PKTS ? n - q * COP_SEG_PKTS : COP_SEG_PKTS;
    return c < cap ? c : cap;
}

static void run(uint32_t n, int layout, uint32_t stride, uint32_t data_off, uint32_t n_lists, int seg,
                const cop_sketch_config *cfg)
{
    const size_t words = (size_t)cfg->rows << cfg->log2_cols;
    uint64_t *ctr = block(8 * words, 8);
    memset(ctr, 0, 8 * words);
    batch t = make(n, layout, stride, data_off, n_lists, seg, cfg->key == COP_SKETCH_KEY_DST);
    for (uint32_t mask = 0; mask < 3; mask++) {
        uint64_t before = 0, after = 0, counting = 0;
        for (size_t w = 0; w < words; w++) before += ctr[w];
        CHECK(cop_sketch_update_host(cfg, ctr, &t.b, 1, mask, 0) == 0);
        for (size_t w = 0; w < words; w++) after += ctr[w];
        for (uint32_t i = 0; i < n; i++)
            counting += t.ipv4[i] && (!mask || ((mask >> t.b.results[i].verdict) & 1));
        CHECK(after - before == counting * cfg->rows);
    }
    /* estimates never below the truth (mask 0 counted every IPv4 packet at least once) */
    uint32_t heavy = 0;
    for (uint32_t i = 0; i < n; i++) heavy += t.ipv4[i] && t.keys[i] == 0x0A010203u;
    uint32_t *ips = block(4 * 3, 4);
    uint64_t *est = block(8 * 3, 8);
    ips[0] = 0x0A010203u, ips[1] = 0x0B000001u, ips[2] = 0xFFFFFFFFu;
    CHECK(cop_sketch_query_host(cfg, ctr, ips, 3, est) == 0);
    CHECK(est[0] >= heavy);
    CHECK(cop_sketch_query_host(cfg, ctr, ips, 0, est) == 0);
    /* police at three thresholds */
    const uint64_t ths[3] = {0, est[0] ? est[0] : 1, UINT64_MAX};
    for (int x = 0; x < 3; x++) {
        t.p.threshold = ths[x];
        CHECK(cop_sketch_police_host(cfg, ctr, &t.b, &t.p, 1, n_lists, seg, 0) == 0);
        if (!n) continue;
        uint32_t kept = 0, total = 0;
        for (uint32_t q = 0; q < t.lists; q++) {
            const uint32_t len = list_len(&t, q, seg);
            CHECK(t.p.out_count[q] <= len);
            if (x == 2) {   /* everything kept, in order */
                CHECK(t.p.out_count[q] == len);
                const size_t first = seg ? (size_t)q * COP_SEG_PKTS : (size_t)q * n;
                CHECK(memcmp(t.p.out_idx + first, t.b.fwd_idx + first, 4 * (size_t)len) == 0);
            }
            kept += t.p.out_count[q];
            total += len;
            if (!seg) CHECK(t.p.status[4 * q] == t.p.out_count[q] && t.p.status[4 * q] + t.p.status[4 * q + 1] == len);
        }
        if (seg) CHECK(t.p.status[0] == kept && t.p.status[1] == total - kept && !t.p.status[2] && !t.p.status[3]);
    }
    /* a refused call: out_idx in place */
    uint32_t *save = t.p.out_idx;
    t.p.out_idx = t.b.fwd_idx;
    CHECK(cop_sketch_police_host(cfg, ctr, &t.b, &t.p, 1, n_lists, seg, 0) == (n ? -EINVAL : 0));
    t.p.out_idx = save;
    free(ips);
    free(est);
    drop(&t);
    free(ctr);
}

int main(void)
{
    const uint32_t ns[] = {0, 1, 63, 255, 256, 257, 1027};
    int k = 0;
    for (size_t x = 0; x < sizeof(ns) / sizeof(ns[0]); x++)
        for (int layout = 0; layout < 3; layout++)
            for (int form = 0; form < 3; form++, k++) {
                const cop_sketch_config cfg = {(k % 2) ? 1u : 4u, (k % 3) ? 10u : 4u, (uint32_t)(k % 2),
                                               (k % 4 == 3) ? 24u : 32u, 77u + (uint64_t)k};
                const uint32_t stride = (k % 2) ? 64 : 2176, data_off = (k % 2) ? 0 : 128;
                run(ns[x], layout, stride, layout == 2 ? 0 : data_off, form == 2 ? 5 : 1, form == 1, &cfg);
            }
    uint32_t a[4], b[4];
    const cop_sketch_config bad = {5, 10, 0, 32, 0};
    CHECK(cop_sketch_params(&bad, a, b) == -EINVAL);
    printf("sketch_check ok (%d runs)\n", k);
    return 0;
}
