/*
 * tx_gather_check.c — stand-alone check of cop_tx_gather_host (tx_gather.c)
 * for the sanitizers: every array is a heap block of exactly the size the
 * semantics allow the call to touch (outputs: cap_bytes, cap_frames words, 4
 * status words; lists: the words the counts cover ... n), so AddressSanitizer
 * stops a byte read or written outside an extent. Each burst is then compared
 * with a frame-by-frame walk of the list.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cop_gpu.h"

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return (uint32_t)(rng >> 16);
}

static void *blk(size_t bytes)   /* 16-byte aligned by malloc; never size 0 */
{
    void *p = malloc(bytes ? bytes : 1);
    if (!p) exit(2);
    memset(p, 0xAB, bytes ? bytes : 1);
    return p;
}

static int fails;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);           \
            fails++;                                                     \
        }                                                                \
    } while (0)

/* form: 0 dense, 1 segmented, 2 demux (K lists); imix: lens cycle; cut: 0 room for all, else caps cut */
static void run(uint32_t n, int form, int imix, uint32_t pct, int cut)
{
    const uint32_t K = form == 2 ? 5 : 1, nseg = (n + 255) / 256;
    const uint32_t stride = 128, data_off = 16, copy = 96, slot = 112;
    static const uint32_t cyc[] = {1, 15, 16, 17, 60, 64, 594, 1518, 2048, 0, 5000};
    uint8_t *pk = blk(imix ? (size_t)n * 64 + 2048 + 16 + data_off : (size_t)n * stride);
    for (size_t i = 0; i < (imix ? (size_t)n * 64 + 2048 + 16 + data_off : (size_t)n * stride); i++) pk[i] = (uint8_t)rnd();
    uint32_t *offsets = imix ? blk((size_t)n * 4) : NULL, *lens = imix ? blk((size_t)n * 4) : NULL;
    for (uint32_t i = 0; imix && i < n; i++) {
        offsets[i] = ((i * 7u) % (n ? n : 1)) * 64u;
        lens[i] = cyc[i % 11];
    }
    /* verdicts and ports, then the lists in their layout */
    uint8_t *fwd = blk(n), *port = blk(n);
    for (uint32_t i = 0; i < n; i++) {
        fwd[i] = rnd() % 100 < pct;
        port[i] = (uint8_t)((i / 64) % K);
    }
    uint32_t *idx = blk((size_t)n * K * 4), *cnt = blk((form == 1 ? (nseg ? nseg : 1) : K) * 4);
    memset(cnt, 0, (form == 1 ? (nseg ? nseg : 1) : K) * 4);
    for (uint32_t i = 0; i < n; i++) {
        if (!fwd[i]) continue;
        if (form == 1) idx[(i / 256) * 256 + cnt[i / 256]++] = i;
        else idx[(size_t)port[i] * n * (form == 2) + cnt[form == 2 ? port[i] : 0]++] = i;
    }
    cop_batch b;
    cop_tx_desc t;
    memset(&b, 0, sizeof(b));
    memset(&t, 0, sizeof(t));
    b.pkts = n ? pk : NULL;
    b.offsets = offsets;   /* an empty IMIX batch is still IMIX (a 1-byte block, never read) */
    b.n = n;
    b.stride = imix ? 0 : stride;
    b.data_off = data_off;
    b.fwd_idx = n ? idx : NULL;
    b.fwd_count = n ? cnt : NULL;
    t.lens = n ? lens : NULL;
    t.copy_bytes = imix ? 0 : copy;
    t.slot_bytes = imix ? 0 : slot;
    uint32_t len_of[8] = {0}, need[8] = {0};
    for (uint32_t q = 0; q < K; q++) {
        /* the list q as a walk of the layout */
        uint32_t L = 0, bytes = 0;
        for (uint32_t i = 0; i < n; i++)
            if (fwd[i] && (form != 2 || port[i] == q)) {
                uint32_t l = imix ? lens[i] : copy;
                l = l < 1 ? 1 : l > 2048 ? 2048 : l;
                bytes = imix ? bytes + ((l + 15) & ~15u) : L * slot + copy;
                L++;
            }
        len_of[q] = L;
        need[q] = bytes;
        cop_tx_burst *o = &t.out[q];
        o->cap_bytes = cut == 0 ? bytes : cut == 1 ? bytes / 2 + 1 : bytes;
        o->cap_frames = cut == 2 ? L / 3 : L;
        o->frames = blk(o->cap_bytes);
        o->off = blk((size_t)o->cap_frames * 4);
        o->len = blk((size_t)o->cap_frames * 4);
        o->status = blk(16);
    }
    const int rc = cop_tx_gather_host(&b, &t, 1, K, form == 1, 0);
    CHECK(rc == 0);
    for (uint32_t q = 0; q < K && rc == 0; q++) {
        const cop_tx_burst *o = &t.out[q];
        const uint32_t W = o->status[0];
        CHECK(W + o->status[2] == len_of[q] && o->status[3] == 0 && W <= o->cap_frames && o->status[1] <= o->cap_bytes);
        if (cut == 0) CHECK(W == len_of[q] && o->status[1] == need[q]);
        uint32_t k = 0, bytes = 0;
        for (uint32_t i = 0; i < n && k < W; i++) {
            if (!fwd[i] || (form == 2 && port[i] != q)) continue;
            uint32_t l = imix ? lens[i] : copy;
            l = l < 1 ? 1 : l > 2048 ? 2048 : l;
            const uint32_t ext = (l + 15) & ~15u, off = imix ? bytes : k * slot;
            const uint8_t *src = pk + (imix ? offsets[i] : i * stride) + data_off;
            CHECK(o->off[k] == off && o->len[k] == l);
            CHECK(memcmp((const uint8_t *)o->frames + off, src, ext) == 0);
            bytes = off + ext;
            k++;
        }
        CHECK(k == W && (W == 0 ? o->status[1] == 0 : o->status[1] == bytes));
        /* the next frame would not have fitted */
        if (W < len_of[q] && !imix) CHECK(W == o->cap_frames || (uint64_t)W * slot + copy > o->cap_bytes);
        free(o->frames);
        free(o->off);
        free(o->len);
        free(o->status);
    }
    free(pk);
    free(offsets);
    free(lens);
    free(fwd);
    free(port);
    free(idx);
    free(cnt);
}

int main(void)
{
    static const uint32_t ns[] = {0, 1, 255, 256, 257, 768, 1027};
    static const uint32_t pcts[] = {0, 2, 50, 98, 100};
    int cases = 0;
    for (unsigned a = 0; a < 7; a++)
        for (int form = 0; form < 3; form++)
            for (int imix = 0; imix < 2; imix++)
                for (unsigned p = 0; p < 5; p++)
                    for (int cut = 0; cut < 3; cut++, cases++) run(ns[a], form, imix, pcts[p], cut);
    /* bad arguments are refused before anything is touched */
    cop_batch b;
    cop_tx_desc t;
    memset(&b, 0, sizeof(b));
    memset(&t, 0, sizeof(t));
    b.n = 4;
    CHECK(cop_tx_gather_host(&b, &t, 1, 1, 0, 0) < 0);
    CHECK(cop_tx_gather_host(NULL, NULL, 0, 1, 0, 0) == 0);
    if (fails) {
        printf("tx_gather_check: %d failures\n", fails);
        return 1;
    }
    printf("tx_gather_check ok: %d cases\n", cases);
    return 0;
}
