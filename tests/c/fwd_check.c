/*
 * fwd_check.c — fwd.c (cop_fwd_check_host, cop_fwd_rewrite_host) over exactly
 * sized heap blocks. Built with -fsanitize=address,undefined by
 * tests/test_fwd_host.py, so a byte read or written outside an extent stops
 * the program; the values are checked against invariants of the specification
 * (include/cop_gpu.h "L3 forward"): kept + removed is the list's length, every
 * removed entry carries a removing class, rewritten + untouched is the frame
 * count, and a rewritten frame of a valid header has a valid checksum, one
 * TTL less and the entry's addresses. Packets end 48 bytes after the last
 * start (IMIX: short frames end after their own extent), the table has
 * exactly n_entries entries, out_idx / exc_idx exactly the list's capacity.
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
            printf("fwd_check: %s failed at line %d\n", #x, __LINE__);     \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static uint64_t rng_state = 0x4321;
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

static void header(uint8_t *f, uint32_t i)
{
    f[12] = 0x08, f[13] = 0x00;
    f[14] = i % 11 == 3 ? 0x46 : i % 13 == 5 ? 0x44 : i % 7 == 6 ? 0x65 : 0x45;
    f[22] = i % 9 == 4 ? (uint8_t)(i & 1) : (uint8_t)(2 + rnd() % 254);
    const uint16_t hc = cop_ipv4_csum_host(f + 14);
    f[24] = (uint8_t)(hc >> 8), f[25] = (uint8_t)hc;
}

static void run(uint32_t n, int imix, uint32_t n_lists, int seg, uint32_t n_entries, uint32_t flags)
{
    const uint32_t segs = (n + COP_SEG_PKTS - 1) / COP_SEG_PKTS, cw = seg ? segs : n_lists;
    cop_neigh_entry *tab = block(sizeof(cop_neigh_entry) * n_entries, 16);
    for (uint32_t e = 0; e < n_entries; e++) {
        for (int j = 0; j < 6; j++) tab[e].dst_mac[j] = (uint8_t)rnd(), tab[e].src_mac[j] = (uint8_t)rnd();
        tab[e].port = (uint16_t)(e & 7);
        tab[e].flags = (uint16_t)((rnd() & 0xFFFE) | (e % 3 != 1));
    }
    cop_batch b;
    memset(&b, 0, sizeof(b));
    uint32_t *offsets = NULL, *lens = NULL;
    uint8_t *pk;
    size_t bytes = 0;
    if (imix) {
        offsets = block(4 * (size_t)n, 4);
        lens = block(4 * (size_t)n, 4);
        for (uint32_t i = 0; i < n; i++) {
            lens[i] = i % 5 == 2 ? 1 + rnd() % 33 : 34 + rnd() % 200;
            offsets[i] = (uint32_t)bytes;
            bytes += (lens[i] + 15) & ~15u;   /* the extent the caller guarantees, and no more */
        }
    } else {
        bytes = (size_t)(n - 1) * 64 + 48;
    }
    pk = block(bytes, 16);
    for (size_t i = 0; i < bytes; i++) pk[i] = (uint8_t)rnd();
    for (uint32_t i = 0; i < n; i++)
        if (!imix || lens[i] >= 34) header(pk + (imix ? offsets[i] : (size_t)i * 64), i);
    cop_result *res = block(8 * (size_t)n, 8);
    for (uint32_t i = 0; i < n; i++) {
        res[i].verdict = 0, res[i].flags = (uint8_t)(rnd() & 3), res[i].port = 0;
        res[i].route_nh = rnd() % (n_entries + 2) | (rnd() << 24);
    }
    /* every packet forwarded, list q takes i % n_lists == q; a few indices past n */
    const size_t idx_words = (size_t)n * (seg ? 1 : n_lists);
    uint32_t *idx = block(4 * idx_words, 16), *cnt = block(4 * (size_t)cw, 4);
    memset(cnt, 0, 4 * (size_t)cw);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t e = i % 17 == 16 ? n + i : i;
        if (seg) idx[(i / COP_SEG_PKTS) * COP_SEG_PKTS + cnt[i / COP_SEG_PKTS]++] = e;
        else idx[(size_t)(i % n_lists) * n + cnt[i % n_lists]++] = e;
    }
    b.pkts = pk, b.offsets = offsets, b.n = n, b.stride = imix ? 0 : 64, b.results = res, b.fwd_idx = idx, b.fwd_count = cnt;
    cop_fwd_check_desc d;
    memset(&d, 0, sizeof(d));
    d.lens = lens;
    d.out_idx = block(4 * idx_words, 16), d.exc_idx = block(4 * idx_words, 16);
    d.out_count = block(4 * (size_t)cw, 4), d.exc_count = block(4 * (size_t)cw, 4);
    d.status = block(16 * (size_t)n_lists, 16);
    const cop_fwd_config cfg = {flags, n_entries > 2 ? 0u : COP_FWD_NO_NH};
    CHECK(cop_fwd_check_host(tab, n_entries, &cfg, &b, &d, 1, n_lists, seg, 0) == 0);
    uint32_t kept = 0, removed = 0, st_kept = 0, st_removed = 0, total = 0;
    for (uint32_t w = 0; w < cw; w++) {
        kept += d.out_count[w], removed += d.exc_count[w], total += cnt[w];
        const size_t first = seg ? (size_t)w * COP_SEG_PKTS : (size_t)w * n;
        for (uint32_t j = 0; j < d.exc_count[w]; j++) {
            const uint32_t e = d.exc_idx[first + j];
            CHECK((e >> 28) >= COP_FWD_SHORT && (e >> 28) <= COP_FWD_NO_NEIGH && (e & 0x0FFFFFFF) < n);
        }
    }
    for (uint32_t q = 0; q < n_lists; q++) st_kept += d.status[4 * q], st_removed += d.status[4 * q + 1];
    CHECK(kept + removed == total && total == n && st_kept == kept && st_removed == removed);

    /* the gather of the kept lists, then the rewrite */
    cop_batch f = b;
    f.fwd_idx = d.out_idx, f.fwd_count = d.out_count;
    cop_tx_desc t;
    cop_fwd_rw_desc r;
    memset(&t, 0, sizeof(t));
    memset(&r, 0, sizeof(r));
    t.lens = lens, t.copy_bytes = imix ? 0 : 48, t.slot_bytes = imix ? 0 : 48;
    for (uint32_t q = 0; q < n_lists; q++) {
        cop_tx_burst *o = &t.out[q];
        o->cap_frames = n;
        o->cap_bytes = imix ? bytes : (uint64_t)n * 48;
        o->frames = block(o->cap_bytes, 16);
        o->off = block(4 * (size_t)n, 4), o->len = block(4 * (size_t)n, 4), o->status = block(16, 16);
        r.port[q] = block(4 * (size_t)n, 4), r.status[q] = block(16, 16);
    }
    CHECK(cop_tx_gather_host(&f, &t, 1, n_lists, seg, 0) == 0);
    uint8_t *before[COP_MAX_DEMUX_PORTS];
    for (uint32_t q = 0; q < n_lists; q++) {
        before[q] = block(t.out[q].status[1], 16);
        memcpy(before[q], t.out[q].frames, t.out[q].status[1]);
    }
    CHECK(cop_fwd_rewrite_host(tab, n_entries, &cfg, &f, &t, &r, 1, n_lists, seg, 0) == 0);
    uint32_t frames = 0, seen = 0;
    for (uint32_t q = 0; q < n_lists; q++) {
        const cop_tx_burst *o = &t.out[q];
        frames += o->status[0];
        seen += r.status[q][0] + r.status[q][1] + r.status[q][2];
        CHECK(r.status[q][2] == 0 && r.status[q][3] == 0);   /* the check removed every other class */
        uint32_t rewritten = 0;
        for (uint32_t k = 0; k < o->status[0]; k++) {
            const uint8_t *was = before[q] + o->off[k], *now = (const uint8_t *)o->frames + o->off[k];
            if (r.port[q][k] == 0xFFFF) {
                CHECK(memcmp(was, now, (o->len[k] + 15) & ~15u) == 0);
                continue;
            }
            rewritten++;
            CHECK(r.port[q][k] < 8 && now[22] == was[22] - 1 && memcmp(was + 26, now + 26, 22) == 0);
            CHECK(memcmp(was + 12, now + 12, 10) == 0 && now[23] == was[23]);
            CHECK(cop_ipv4_csum_host(now + 14) == (uint16_t)((now[24] << 8) | now[25]));
        }
        CHECK(rewritten == r.status[q][0]);
    }
    CHECK(frames == kept && seen == frames);

    free(tab), free(offsets), free(lens), free(pk), free(res), free(idx), free(cnt);
    free(d.out_idx), free(d.exc_idx), free(d.out_count), free(d.exc_count), free(d.status);
    for (uint32_t q = 0; q < n_lists; q++) {
        free(t.out[q].frames), free(t.out[q].off), free(t.out[q].len), free(t.out[q].status);
        free(r.port[q]), free(r.status[q]), free(before[q]);
    }
}

int main(void)
{
    const uint32_t ns[] = {1, 63, 256, 257, 1027};
    for (unsigned a = 0; a < sizeof(ns) / sizeof(ns[0]); a++)
        for (int imix = 0; imix < 2; imix++)
            for (uint32_t flags = 0; flags < 2; flags++) {
                run(ns[a], imix, 1, 0, 1 + a * 7, flags);
                run(ns[a], imix, 1, 1, 1u << (a + 2), flags);
                run(ns[a], imix, 3, 0, 5, flags);
            }
    printf("fwd_check ok\n");
    return 0;
}
