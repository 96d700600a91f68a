/*
 * aead_check.c — aead.c (cop_aead_*_host, cop_poly1305_host,
 * cop_chacha20_block_host) over exactly sized heap blocks. Built with
 * -fsanitize=address,undefined by tests/test_aead_host.py, so a byte read or
 * written outside an extent stops the program; the values are checked against
 * the RFC 8439 vectors and invariants of the specification (include/cop_gpu.h
 * "AEAD"): the associated data stay in clear, seal then open restores every
 * byte, a flipped bit fails exactly its frame and leaves it as it was,
 * processed + skipped is the number of frames present.
 */
#define _POSIX_C_SOURCE 200112L
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cop_gpu.h"

#define CHECK(x)                                                            \
    do {                                                                    \
        if (!(x)) {                                                         \
            printf("aead_check: %s failed at line %d\n", #x, __LINE__);     \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static uint64_t rng_state = 0xAEAD;
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

static void rfc_vectors(void)
{
    static const char text[] = "Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the "
                               "future, sunscreen would be it.";
    static const uint8_t aad[12] = {0x50, 0x51, 0x52, 0x53, 0xc0, 0xc1, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7};
    static const uint8_t ct16[16] = {0xd3, 0x1a, 0x8d, 0x34, 0x64, 0x8e, 0x60, 0xdb, 0x7b, 0x86, 0xaf, 0xbc, 0x53, 0xef, 0x7e, 0xc2};
    static const uint8_t want[16] = {0x1a, 0xe1, 0x0b, 0x59, 0x4f, 0x09, 0xe2, 0x6a, 0x7e, 0x90, 0x2e, 0xcb, 0xd0, 0x60, 0x06, 0x91};
    cop_aead_key key;
    memset(&key, 0, sizeof(key));
    for (int i = 0; i < 32; i++) key.key[i] = (uint8_t)(0x80 + i);
    key.salt[0] = 7;
    const uint32_t l = 12 + 114;
    CHECK(sizeof(text) - 1 == 114);
    uint8_t *f = block(128, 16);            /* ext = 128: not a byte more */
    uint8_t *tags = block(16, 16);
    uint32_t *status = block(16, 16), *off = block(4, 4), *len = block(4, 4), *ok = block(4, 4);
    memcpy(f, aad, 12);
    memcpy(f + 12, text, 114);
    f[126] = f[127] = 0xEE;
    off[0] = 0, len[0] = l;
    cop_aead_burst b;
    memset(&b, 0, sizeof(b));
    b.frames = f, b.off = off, b.len = len, b.tags = tags, b.status = status;
    b.cap_bytes = 128, b.seq_base = 0x4746454443424140ull, b.n_frames = 1, b.aad_bytes = 12;
    CHECK(cop_aead_seal_host(&key, &b, 1) == 0);
    CHECK(!memcmp(f, aad, 12) && !memcmp(f + 12, ct16, 16) && !memcmp(tags, want, 16));
    CHECK(f[126] == 0xEE && f[127] == 0xEE);
    CHECK(status[0] == 1 && status[1] == 0 && status[2] == 0 && status[3] == 0);
    b.ok = ok;
    CHECK(cop_aead_open_host(&key, &b, 1) == 0);
    CHECK(ok[0] == 1 && !memcmp(f + 12, text, 114) && status[0] == 1 && status[1] == 0);
    free(f), free(tags), free(status), free(off), free(len), free(ok);

    /* RFC 8439 2.5.2 and 2.3.2 */
    static const uint8_t otk[32] = {0x85, 0xd6, 0xbe, 0x78, 0x57, 0x55, 0x6d, 0x33, 0x7f, 0x44, 0x52, 0xfe, 0x42, 0xd5, 0x06, 0xa8,
                                    0x01, 0x03, 0x80, 0x8a, 0xfb, 0x0d, 0xb2, 0xfd, 0x4a, 0xbf, 0xf6, 0xaf, 0x41, 0x49, 0xf5, 0x1b};
    static const uint8_t ptag[16] = {0xa8, 0x06, 0x1d, 0xc1, 0x30, 0x51, 0x36, 0xc6, 0xc2, 0x2b, 0x8b, 0xaf, 0x0c, 0x01, 0x27, 0xa9};
    const char *m = "Cryptographic Forum Research Group";
    uint8_t *msg = block(34, 1), *t = block(16, 1);
    memcpy(msg, m, 34);
    cop_poly1305_host(otk, msg, 34, t);
    CHECK(!memcmp(t, ptag, 16));
    cop_poly1305_host(otk, msg, 0, t);          /* no byte of msg is read */
    CHECK(!memcmp(t, otk + 16, 16));
    free(msg), free(t);
    uint8_t k[32], nonce[12] = {0, 0, 0, 9, 0, 0, 0, 0x4a, 0, 0, 0, 0}, *out = block(64, 1);
    for (int i = 0; i < 32; i++) k[i] = (uint8_t)i;
    cop_chacha20_block_host(k, 1, nonce, out);
    CHECK(out[0] == 0x10 && out[1] == 0xf1 && out[2] == 0xe7 && out[3] == 0xe4 && out[63] == 0x4e);
    free(out);
}

/* a burst of n frames of every length kind; form 0: slot, 1: off / len with a misaligned and an
 * overhanging frame in the middle */
static void burst(uint32_t n, int form, uint32_t aad, uint32_t frame_bytes, const uint32_t *count_val)
{
    static const uint32_t kinds[] = {1, 15, 16, 17, 60, 64, 65, 127, 129, 594, 1518, 2048, 5000, 0};
    cop_aead_key key;
    memset(&key, 0, sizeof(key));
    for (int i = 0; i < 32; i++) key.key[i] = (uint8_t)rnd();
    for (int i = 0; i < 4; i++) key.salt[i] = (uint8_t)rnd();
    const uint32_t m = n ? n : 1;
    uint32_t *off = NULL, *len = NULL, *count = NULL;
    uint64_t cap = 0;
    const uint32_t slot = (frame_bytes + 15u) & ~15u;
    if (form) {
        off = block(4 * (size_t)m, 4), len = block(4 * (size_t)m, 4);
        for (uint32_t k = 0; k < n; k++) {
            len[k] = kinds[rnd() % (sizeof(kinds) / sizeof(kinds[0]))];
            const uint32_t l = len[k] > COP_TX_MAX_FRAME ? COP_TX_MAX_FRAME : len[k];
            off[k] = (uint32_t)cap;
            cap += (l + 15u) & ~15u;
        }
        if (n > 8) {
            off[3] += 4;                      /* misaligned */
            off[5] = (uint32_t)cap - 16;      /* does not fit unless it is short */
            len[5] = 64;
        }
    } else {
        cap = (uint64_t)n * slot;
    }
    if (count_val) {
        count = block(4, 4);
        *count = *count_val;
    }
    uint8_t *f = block(cap, 16), *orig = block(cap, 16), *sealed = block(cap, 16);
    for (uint64_t i = 0; i < cap; i++) f[i] = orig[i] = (uint8_t)rnd();
    uint8_t *tags = block(16 * (size_t)m, 16);
    memset(tags, 0xAB, 16 * (size_t)m);
    uint32_t *ok = block(4 * (size_t)m, 4), *status = block(16, 16);
    memset(ok, 0xAB, 4 * (size_t)m);
    cop_aead_burst b;
    memset(&b, 0, sizeof(b));
    b.frames = f, b.off = off, b.len = len, b.count = count, b.tags = tags, b.status = status;
    b.cap_bytes = cap, b.seq_base = ~0ull - 2, b.n_frames = n, b.aad_bytes = aad;
    if (!form) b.slot_bytes = slot, b.frame_bytes = frame_bytes;
    status[0] = status[1] = status[2] = status[3] = 0xABABABABu;
    CHECK(cop_aead_seal_host(&key, &b, 1) == 0);
    const uint32_t present = count && *count < n ? *count : n;
    if (n) CHECK(status[0] + status[2] == present && status[1] == 0 && status[3] == 0);
    else CHECK(status[0] == 0xABABABABu);
    if (form && n > 8 && present > 5) CHECK(status[2] == 2);
    /* the associated data stay in clear; something of every text changed */
    for (uint32_t k = 0; k < present && !form; k++)
        CHECK(!memcmp(f + (size_t)k * slot, orig + (size_t)k * slot, aad < frame_bytes ? aad : frame_bytes));
    if (!form) {
        for (uint32_t k = present; k < n; k++) CHECK(!memcmp(f + (size_t)k * slot, orig + (size_t)k * slot, slot));
        for (uint32_t k = present; k < n; k++) CHECK(tags[16 * (size_t)k] == 0xAB && tags[16 * (size_t)k + 15] == 0xAB);
    }
    memcpy(sealed, f, cap);
    /* a flipped bit in frame 1 (text or, with no text, the associated data) */
    const int flip = !form && present > 1;
    if (flip) f[slot + frame_bytes - 1] ^= 0x10;
    b.ok = ok;
    CHECK(cop_aead_open_host(&key, &b, 1) == 0);
    if (n) CHECK(status[0] + status[2] == present && status[1] == (uint32_t)flip);
    if (flip) {
        CHECK(ok[1] == 0 && ok[0] == 1);
        CHECK(f[slot + frame_bytes - 1] == (sealed[slot + frame_bytes - 1] ^ 0x10));
        f[slot + frame_bytes - 1] ^= 0x10;
        CHECK(!memcmp(f + slot, sealed + slot, slot));   /* the forged frame is as it was */
        memcpy(f + slot, orig + slot, slot);
    }
    CHECK(!memcmp(f, orig, cap));                        /* every other byte is restored */
    free(f), free(orig), free(sealed), free(tags), free(ok), free(status), free(off), free(len), free(count);
}

static void errors(void)
{
    cop_aead_key key;
    memset(&key, 0, sizeof(key));
    uint8_t *f = block(256, 16), *tags = block(64, 16);
    uint32_t *status = block(16, 16), *ok = block(16, 4);
    cop_aead_burst b;
    memset(&b, 0, sizeof(b));
    b.frames = f, b.tags = tags, b.status = status, b.cap_bytes = 256, b.n_frames = 4, b.slot_bytes = 64, b.frame_bytes = 64;
    memset(f, 1, 256);
    cop_aead_burst t = b;
    t.ok = ok;
    CHECK(cop_aead_seal_host(&key, &t, 1) == -EINVAL);
    t = b;
    CHECK(cop_aead_open_host(&key, &t, 1) == -EINVAL);      /* no ok */
    t.frame_bytes = 65;
    CHECK(cop_aead_seal_host(&key, &t, 1) == -EINVAL);
    t = b, t.tags = f + 64;
    CHECK(cop_aead_seal_host(&key, &t, 1) == -EINVAL);
    t = b, t.cap_bytes = 1ull << 32;
    CHECK(cop_aead_seal_host(&key, &t, 1) == -EINVAL);
    for (int i = 0; i < 256; i++) CHECK(f[i] == 1);
    CHECK(cop_aead_seal_host(&key, NULL, 0) == 0);
    t = b, t.n_frames = 0, t.frames = NULL, t.tags = NULL, t.status = NULL;
    CHECK(cop_aead_seal_host(&key, &t, 1) == 0);
    free(f), free(tags), free(status), free(ok);
}

int main(void)
{
    rfc_vectors();
    static const uint32_t ns[] = {0, 1, 63, 64, 65, 257};
    const uint32_t below = 40, above = 1000;
    for (unsigned i = 0; i < sizeof(ns) / sizeof(ns[0]); i++) {
        burst(ns[i], 0, 34, 64, NULL);
        burst(ns[i], 0, 14, 2048, NULL);
        burst(ns[i], 0, 64, 17, NULL);       /* aad >= l: authenticated only */
        burst(ns[i], 0, 0, 1, &below);
        burst(ns[i], 1, 34, 0, NULL);
        burst(ns[i], 1, 0, 0, &above);
        burst(ns[i], 1, 12, 0, &below);
    }
    errors();
    printf("aead_check ok\n");
    return 0;
}
