/*
 * aead.c — cop_aead_*_host: ChaCha20-Poly1305 (RFC 8439) over the frames of tx
 * bursts in host memory, the mirror of the device kernels (cop_aead.hip); the
 * argument checks both share (include/cop_gpu.h "AEAD"); and the two building
 * blocks, cop_chacha20_block_host and cop_poly1305_host.
 *
 * Poly1305 is kept in five 26-bit limbs with 32 x 32 -> 64 products, as the
 * device kernel keeps it, so the two carry chains are the same code.
 *
 * The ChaCha block counter of a frame runs from 0 (the one-time key) to at
 * most 1 + COP_TX_MAX_FRAME / 64 - 1 = 32: it never wraps.
 */
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "cop_internal.h"

/* ---- ChaCha20 ---------------------------------------------------------------- */
static uint32_t le32(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

static void put32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8), p[2] = (uint8_t)(v >> 16), p[3] = (uint8_t)(v >> 24);
}

static uint32_t rotl(uint32_t v, int n)
{
    return (v << n) | (v >> (32 - n));
}

#define QR(a, b, c, d)                 \
    do {                               \
        a += b, d ^= a, d = rotl(d, 16); \
        c += d, b ^= c, b = rotl(b, 12); \
        a += b, d ^= a, d = rotl(d, 8);  \
        c += d, b ^= c, b = rotl(b, 7);  \
    } while (0)

void cop_chacha20_block_host(const uint8_t key[32], uint32_t counter, const uint8_t nonce[12], uint8_t out[64])
{
    uint32_t s[16], x[16];
    s[0] = 0x61707865u, s[1] = 0x3320646eu, s[2] = 0x79622d32u, s[3] = 0x6b206574u;
    for (int i = 0; i < 8; i++) s[4 + i] = le32(key + 4 * i);
    s[12] = counter;
    for (int i = 0; i < 3; i++) s[13 + i] = le32(nonce + 4 * i);
    memcpy(x, s, sizeof(x));
    for (int r = 0; r < 10; r++) {
        QR(x[0], x[4], x[8], x[12]);
        QR(x[1], x[5], x[9], x[13]);
        QR(x[2], x[6], x[10], x[14]);
        QR(x[3], x[7], x[11], x[15]);
        QR(x[0], x[5], x[10], x[15]);
        QR(x[1], x[6], x[11], x[12]);
        QR(x[2], x[7], x[8], x[13]);
        QR(x[3], x[4], x[9], x[14]);
    }
    for (int i = 0; i < 16; i++) put32(out + 4 * i, x[i] + s[i]);
}

/* ---- Poly1305, 26-bit limbs ---------------------------------------------------- */
typedef struct {
    uint32_t r[5], h[5], pad[4];
} poly;

static void poly_init(poly *p, const uint8_t otk[32])
{
    const uint32_t t0 = le32(otk), t1 = le32(otk + 4), t2 = le32(otk + 8), t3 = le32(otk + 12);
    p->r[0] = t0 & 0x3ffffffu;
    p->r[1] = ((t0 >> 26) | (t1 << 6)) & 0x3ffff03u;
    p->r[2] = ((t1 >> 20) | (t2 << 12)) & 0x3ffc0ffu;
    p->r[3] = ((t2 >> 14) | (t3 << 18)) & 0x3f03fffu;
    p->r[4] = (t3 >> 8) & 0x00fffffu;
    for (int i = 0; i < 5; i++) p->h[i] = 0;
    for (int i = 0; i < 4; i++) p->pad[i] = le32(otk + 16 + 4 * i);
}

/* h = (h + block) * r mod 2^130 - 5; hibit: 1 << 24 for a full block, 0 for a final partial one */
static void poly_block(poly *p, const uint8_t m[16], uint32_t hibit)
{
    const uint32_t r0 = p->r[0], r1 = p->r[1], r2 = p->r[2], r3 = p->r[3], r4 = p->r[4];
    const uint32_t s1 = r1 * 5, s2 = r2 * 5, s3 = r3 * 5, s4 = r4 * 5;
    const uint32_t t0 = le32(m), t1 = le32(m + 4), t2 = le32(m + 8), t3 = le32(m + 12);
    uint32_t h0 = p->h[0], h1 = p->h[1], h2 = p->h[2], h3 = p->h[3], h4 = p->h[4], c;
    h0 += t0 & 0x3ffffffu;
    h1 += ((t0 >> 26) | (t1 << 6)) & 0x3ffffffu;
    h2 += ((t1 >> 20) | (t2 << 12)) & 0x3ffffffu;
    h3 += ((t2 >> 14) | (t3 << 18)) & 0x3ffffffu;
    h4 += (t3 >> 8) | hibit;
    uint64_t d0 = (uint64_t)h0 * r0 + (uint64_t)h1 * s4 + (uint64_t)h2 * s3 + (uint64_t)h3 * s2 + (uint64_t)h4 * s1;
    uint64_t d1 = (uint64_t)h0 * r1 + (uint64_t)h1 * r0 + (uint64_t)h2 * s4 + (uint64_t)h3 * s3 + (uint64_t)h4 * s2;
    uint64_t d2 = (uint64_t)h0 * r2 + (uint64_t)h1 * r1 + (uint64_t)h2 * r0 + (uint64_t)h3 * s4 + (uint64_t)h4 * s3;
    uint64_t d3 = (uint64_t)h0 * r3 + (uint64_t)h1 * r2 + (uint64_t)h2 * r1 + (uint64_t)h3 * r0 + (uint64_t)h4 * s4;
    uint64_t d4 = (uint64_t)h0 * r4 + (uint64_t)h1 * r3 + (uint64_t)h2 * r2 + (uint64_t)h3 * r1 + (uint64_t)h4 * r0;
    c = (uint32_t)(d0 >> 26), h0 = (uint32_t)d0 & 0x3ffffffu, d1 += c;
    c = (uint32_t)(d1 >> 26), h1 = (uint32_t)d1 & 0x3ffffffu, d2 += c;
    c = (uint32_t)(d2 >> 26), h2 = (uint32_t)d2 & 0x3ffffffu, d3 += c;
    c = (uint32_t)(d3 >> 26), h3 = (uint32_t)d3 & 0x3ffffffu, d4 += c;
    c = (uint32_t)(d4 >> 26), h4 = (uint32_t)d4 & 0x3ffffffu, h0 += c * 5;
    c = h0 >> 26, h0 &= 0x3ffffffu, h1 += c;
    p->h[0] = h0, p->h[1] = h1, p->h[2] = h2, p->h[3] = h3, p->h[4] = h4;
}

/* n bytes as full blocks, a tail of 1..15 bytes zero-padded to one more full block (pad16) */
static void poly_padded(poly *p, const uint8_t *m, size_t n)
{
    for (; n >= 16; m += 16, n -= 16) poly_block(p, m, 1u << 24);
    if (n) {
        uint8_t b[16] = {0};
        memcpy(b, m, n);
        poly_block(p, b, 1u << 24);
    }
}

static void poly_finish(poly *p, uint8_t tag[16])
{
    uint32_t h0 = p->h[0], h1 = p->h[1], h2 = p->h[2], h3 = p->h[3], h4 = p->h[4], c;
    c = h1 >> 26, h1 &= 0x3ffffffu, h2 += c;
    c = h2 >> 26, h2 &= 0x3ffffffu, h3 += c;
    c = h3 >> 26, h3 &= 0x3ffffffu, h4 += c;
    c = h4 >> 26, h4 &= 0x3ffffffu, h0 += c * 5;
    c = h0 >> 26, h0 &= 0x3ffffffu, h1 += c;
    /* g = h + 5 - 2^130; h >= p iff g did not borrow */
    uint32_t g0 = h0 + 5, g1, g2, g3, g4;
    c = g0 >> 26, g0 &= 0x3ffffffu;
    g1 = h1 + c, c = g1 >> 26, g1 &= 0x3ffffffu;
    g2 = h2 + c, c = g2 >> 26, g2 &= 0x3ffffffu;
    g3 = h3 + c, c = g3 >> 26, g3 &= 0x3ffffffu;
    g4 = h4 + c - (1u << 26);
    const uint32_t take_g = (g4 >> 31) - 1u; /* all ones iff no borrow */
    h0 = (h0 & ~take_g) | (g0 & take_g);
    h1 = (h1 & ~take_g) | (g1 & take_g);
    h2 = (h2 & ~take_g) | (g2 & take_g);
    h3 = (h3 & ~take_g) | (g3 & take_g);
    h4 = (h4 & ~take_g) | (g4 & take_g);
    /* h mod 2^128 as four words, plus s */
    const uint32_t w0 = h0 | (h1 << 26), w1 = (h1 >> 6) | (h2 << 20), w2 = (h2 >> 12) | (h3 << 14),
                   w3 = (h3 >> 18) | (h4 << 8);
    uint64_t f = (uint64_t)w0 + p->pad[0];
    put32(tag, (uint32_t)f);
    f = (uint64_t)w1 + p->pad[1] + (f >> 32);
    put32(tag + 4, (uint32_t)f);
    f = (uint64_t)w2 + p->pad[2] + (f >> 32);
    put32(tag + 8, (uint32_t)f);
    f = (uint64_t)w3 + p->pad[3] + (f >> 32);
    put32(tag + 12, (uint32_t)f);
}

void cop_poly1305_host(const uint8_t otk[32], const uint8_t *msg, size_t n, uint8_t tag[16])
{
    poly p;
    poly_init(&p, otk);
    for (; n >= 16; msg += 16, n -= 16) poly_block(&p, msg, 1u << 24);
    if (n) {
        uint8_t b[16] = {0};
        memcpy(b, msg, n);
        b[n] = 1;
        poly_block(&p, b, 0);
    }
    poly_finish(&p, tag);
}

/* ---- argument checks ----------------------------------------------------------- */
int cop_aead_validate(const cop_aead_key *key, const cop_aead_burst *bursts, uint32_t nb, int mode, const uint8_t *otk,
                      uint32_t max_batch, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "null argument";
    if ((mode != COP_AEAD_MODE_POLY && !key) || (nb && !bursts)) return -EINVAL;
    uint32_t live = 0;
    for (uint32_t i = 0; i < nb; i++) {
        const cop_aead_burst *b = &bursts[i];
        *why = "n_frames > max_batch";
        if (max_batch && b->n_frames > max_batch) return -EINVAL;
        if (!b->n_frames) continue;
        live++;
        *why = "a burst with frames needs frames, tags and status (open: ok; poly1305_bulk: otk)";
        if (!b->frames || !b->tags || !b->status || (mode == COP_AEAD_MODE_OPEN && !b->ok) ||
            (mode == COP_AEAD_MODE_POLY && !otk))
            return -EINVAL;
        *why = "ok is written by open alone: NULL otherwise";
        if (mode != COP_AEAD_MODE_OPEN && b->ok) return -EINVAL;
        *why = "off and len: both or neither";
        if (!b->off != !b->len) return -EINVAL;
        if (!b->off) {
            *why = "slot form: frame_bytes 1..COP_TX_MAX_FRAME, slot_bytes a multiple of 16 >= frame_bytes";
            if (b->frame_bytes < 1 || b->frame_bytes > COP_TX_MAX_FRAME || (b->slot_bytes & 15) ||
                b->slot_bytes < b->frame_bytes)
                return -EINVAL;
        }
        *why = "aad_bytes > COP_TX_MAX_FRAME";
        if (b->aad_bytes > COP_TX_MAX_FRAME) return -EINVAL;
        *why = "frames, tags and status must be 16-byte aligned; off, len, count and ok 4-byte aligned";
        if ((((uintptr_t)b->frames | (uintptr_t)b->tags | (uintptr_t)b->status) & 15) ||
            (((uintptr_t)b->off | (uintptr_t)b->len | (uintptr_t)b->count | (uintptr_t)b->ok | (uintptr_t)otk) & 3))
            return -EINVAL;
        *why = "cap_bytes >= 2^32";
        if (b->cap_bytes >= (1ull << 32)) return -EINVAL;
    }
    if (!live) {
        *why = "";
        return 0;
    }
    /* nothing the call writes (frames, tags, ok, status) over any other extent of any burst */
    cop_extent *e = (cop_extent *)malloc((size_t)live * 8 * sizeof(cop_extent));
    *why = "out of memory";
    if (!e) return -ENOMEM;
    uint32_t ne = 0;
    for (uint32_t i = 0; i < nb; i++) {
        const cop_aead_burst *b = &bursts[i];
        const uint64_t n = b->n_frames;
        if (!n) continue;
        cop_extent_put(e, &ne, b->frames, b->cap_bytes, 1);
        cop_extent_put(e, &ne, b->tags, 16 * n, 1);
        cop_extent_put(e, &ne, b->ok, 4 * n, 1);
        cop_extent_put(e, &ne, b->status, 16, 1);
        cop_extent_put(e, &ne, b->off, 4 * n, 0);
        cop_extent_put(e, &ne, b->len, 4 * n, 0);
        cop_extent_put(e, &ne, b->count, 4, 0);
        if (mode == COP_AEAD_MODE_POLY) cop_extent_put(e, &ne, otk, 32 * n, 0);
    }
    const int rc = cop_extents_clash(e, ne, 0) ? -EINVAL : 0;
    free(e);
    *why = rc ? "frames, tags, ok or status overlaps another extent of the call" : "";
    return rc;
}

/* ---- the mirror ------------------------------------------------------------------ */
/* frame k of the burst: 0 and (o, l) if it is processed, 1 if skipped */
static int frame_of(const cop_aead_burst *b, uint32_t k, uint32_t *o, uint32_t *l)
{
    uint32_t len = b->off ? b->len[k] : b->frame_bytes;
    if (len > COP_TX_MAX_FRAME) len = COP_TX_MAX_FRAME;
    const uint64_t off = b->off ? (uint64_t)b->off[k] : (uint64_t)k * b->slot_bytes;
    const uint32_t ext = (len + 15u) & ~15u;
    if ((off & 15) || off + ext > b->cap_bytes) return 1;
    *o = (uint32_t)off;
    *l = len;
    return 0;
}

static uint32_t frames_present(const cop_aead_burst *b)
{
    return b->count && *b->count < b->n_frames ? *b->count : b->n_frames;
}

static void nonce_of(const cop_aead_key *key, uint64_t seq, uint8_t nonce[12])
{
    memcpy(nonce, key->salt, 4);
    for (int i = 0; i < 8; i++) nonce[4 + i] = (uint8_t)(seq >> (8 * i));
}

static void xor_stream(const cop_aead_key *key, const uint8_t nonce[12], uint8_t *text, uint32_t n)
{
    uint8_t ks[64];
    for (uint32_t at = 0, ctr = 1; at < n; at += 64, ctr++) {   /* ctr <= 32 */
        cop_chacha20_block_host(key->key, ctr, nonce, ks);
        const uint32_t m = n - at < 64 ? n - at : 64;
        for (uint32_t i = 0; i < m; i++) text[at + i] ^= ks[i];
    }
}

static void frame_tag(const cop_aead_key *key, const uint8_t nonce[12], const uint8_t *f, uint32_t a, uint32_t l,
                      uint8_t tag[16])
{
    uint8_t b0[64], lens[16] = {0};
    poly p;
    cop_chacha20_block_host(key->key, 0, nonce, b0);
    poly_init(&p, b0);
    poly_padded(&p, f, a);
    poly_padded(&p, f + a, l - a);
    put32(lens, a);
    put32(lens + 8, l - a);
    poly_block(&p, lens, 1u << 24);
    poly_finish(&p, tag);
}

static int aead_host(const cop_aead_key *key, const cop_aead_burst *bursts, uint32_t nb, int mode)
{
    if (nb == 0) return 0;
    if (cop_aead_validate(key, bursts, nb, mode, NULL, 0, NULL)) return -EINVAL;
    for (uint32_t i = 0; i < nb; i++) {
        const cop_aead_burst *b = &bursts[i];
        if (!b->n_frames) continue;
        const uint32_t n = frames_present(b);
        uint32_t done = 0, bad = 0, skipped = 0;
        for (uint32_t k = 0; k < n; k++) {
            uint32_t o, l;
            if (frame_of(b, k, &o, &l)) {
                skipped++;
                continue;
            }
            uint8_t *f = (uint8_t *)b->frames + o, nonce[12], tag[16];
            const uint32_t a = b->aad_bytes < l ? b->aad_bytes : l;
            nonce_of(key, b->seq_base + k, nonce);
            done++;
            if (mode == COP_AEAD_MODE_SEAL) {
                xor_stream(key, nonce, f + a, l - a);
                frame_tag(key, nonce, f, a, l, b->tags + 16 * (size_t)k);
                continue;
            }
            frame_tag(key, nonce, f, a, l, tag);
            uint8_t diff = 0;
            for (int j = 0; j < 16; j++) diff |= (uint8_t)(tag[j] ^ b->tags[16 * (size_t)k + j]);
            b->ok[k] = diff == 0;
            if (diff) bad++;
            else xor_stream(key, nonce, f + a, l - a);
        }
        b->status[0] = done;
        b->status[1] = bad;
        b->status[2] = skipped;
        b->status[3] = 0;
    }
    return 0;
}

int cop_aead_seal_host(const cop_aead_key *key, const cop_aead_burst *bursts, uint32_t nb)
{
    return aead_host(key, bursts, nb, COP_AEAD_MODE_SEAL);
}

int cop_aead_open_host(const cop_aead_key *key, const cop_aead_burst *bursts, uint32_t nb)
{
    return aead_host(key, bursts, nb, COP_AEAD_MODE_OPEN);
}
