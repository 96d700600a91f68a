/*
 * sketch.c — cop_sketch_*_host: the count-min sketch over host memory, the
 * mirror of the device kernels (cop_sketch.hip), and the argument checks both
 * share (include/cop_gpu.h "Sketch").
 *
 * The police mirror walks every list the way the kernels cut it up: in chunks
 * of COP_SEG_PKTS positions (a segment; positions 256c .. of a dense or
 * per-vport list). It writes what the kernels write and nothing else.
 */
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "cop_internal.h"

static uint64_t sm64(uint64_t *s)
{
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int cop_sketch_config_check(const cop_sketch_config *cfg, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "null config";
    if (!cfg) return -EINVAL;
    *why = "rows must be 1..COP_SKETCH_MAX_ROWS";
    if (cfg->rows < 1 || cfg->rows > COP_SKETCH_MAX_ROWS) return -EINVAL;
    *why = "log2_cols must be 4..24";
    if (cfg->log2_cols < 4 || cfg->log2_cols > 24) return -EINVAL;
    *why = "key must be COP_SKETCH_KEY_SRC or COP_SKETCH_KEY_DST";
    if (cfg->key > COP_SKETCH_KEY_DST) return -EINVAL;
    *why = "key_depth must be 1..32";
    if (cfg->key_depth < 1 || cfg->key_depth > 32) return -EINVAL;
    *why = "";
    return 0;
}

int cop_sketch_params(const cop_sketch_config *cfg, uint32_t a[4], uint32_t b[4])
{
    if (!a || !b || cop_sketch_config_check(cfg, NULL)) return -EINVAL;
    uint64_t s = cfg->seed;
    for (uint32_t r = 0; r < COP_SKETCH_MAX_ROWS; r++) {
        const uint64_t z = r < cfg->rows ? sm64(&s) : 0;
        a[r] = r < cfg->rows ? ((uint32_t)z | 1u) : 0u;
        b[r] = (uint32_t)(z >> 32);
    }
    return 0;
}

/* what a sketch call reads of a batch's packets: the checks update and police share */
static int batch_packets_check(const cop_batch *b, uint32_t max_batch, const char **why)
{
    *why = "n > max_batch";
    if (max_batch && b->n > max_batch) return -EINVAL;
    *why = "a batch with packets needs pkts";
    if (b->n && !b->pkts) return -EINVAL;
    *why = "packet starts must be 16-byte aligned (pkts, data_off, stride; 12-byte records are not taken)";
    if (cop_batch_misaligned(b)) return -EINVAL;
    *why = "stride must be COP_HDR16_STRIDE (records) or at least 48 (frames)";
    if (!b->offsets && b->n && b->stride != COP_HDR16_STRIDE && b->stride < 48) return -EINVAL;
    *why = "offsets must be 4-byte aligned";
    if ((uintptr_t)b->offsets & 3) return -EINVAL;
    return 0;
}

int cop_sketch_update_validate(const cop_batch *batches, uint32_t nb, uint32_t verdict_mask, uint32_t max_batch,
                               const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "null argument";
    if (nb && !batches) return -EINVAL;
    *why = "verdict_mask has bits above COP_DROP_NO_PORT";
    if (verdict_mask >> (COP_DROP_NO_PORT + 1)) return -EINVAL;
    for (uint32_t i = 0; i < nb; i++) {
        const cop_batch *b = &batches[i];
        if (batch_packets_check(b, max_batch, why)) return -EINVAL;
        *why = "verdict_mask != 0 needs results (8-byte aligned)";
        if (verdict_mask && b->n && (!b->results || ((uintptr_t)b->results & 7))) return -EINVAL;
    }
    *why = "";
    return 0;
}

int cop_sketch_query_validate(const cop_sketch_config *cfg, const void *counters, const uint32_t *ips, uint32_t n,
                              const uint64_t *out, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    if (cop_sketch_config_check(cfg, why)) return -EINVAL;
    *why = "null argument";
    if (!counters || (n && (!ips || !out))) return -EINVAL;
    *why = "ips must be 4-byte aligned, out 8-byte aligned";
    if (((uintptr_t)ips & 3) || ((uintptr_t)out & 7)) return -EINVAL;
    *why = "out overlaps ips or the counters";
    cop_extent v[3];
    uint32_t k = 0;
    cop_extent_put(v, &k, out, 8ull * n, 1);
    cop_extent_put(v, &k, ips, 4ull * n, 0);
    cop_extent_put(v, &k, counters, ((uint64_t)cfg->rows << cfg->log2_cols) * 8, 0);
    if (cop_extents_clash(v, k, 0)) return -EINVAL;
    *why = "";
    return 0;
}

int cop_sketch_police_validate(const cop_sketch_config *cfg, const void *counters, const cop_batch *batches,
                               const cop_police_desc *pol, uint32_t nb, uint32_t n_lists, int seg,
                               uint32_t max_batch, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    if (cop_sketch_config_check(cfg, why)) return -EINVAL;
    *why = "null argument";
    if (!counters || (nb && (!batches || !pol))) return -EINVAL;
    *why = "list layout: 1..COP_MAX_DEMUX_PORTS lists per batch, segmented lists one";
    if (n_lists < 1 || n_lists > COP_MAX_DEMUX_PORTS || (seg && n_lists != 1)) return -EINVAL;
    for (uint32_t i = 0; i < nb; i++) {
        const cop_batch *b = &batches[i];
        const cop_police_desc *p = &pol[i];
        if (batch_packets_check(b, max_batch, why)) return -EINVAL;
        *why = "a batch with packets needs fwd_idx, fwd_count, out_idx, out_count and status";
        if (b->n && (!b->fwd_idx || !b->fwd_count || !p->out_idx || !p->out_count || !p->status)) return -EINVAL;
        *why = "fwd_idx / fwd_count / out_idx / out_count must be 4-byte aligned, status 16-byte aligned";
        if ((((uintptr_t)b->fwd_idx | (uintptr_t)b->fwd_count | (uintptr_t)p->out_idx | (uintptr_t)p->out_count) & 3) ||
            ((uintptr_t)p->status & 15))
            return -EINVAL;
    }
    /* no output extent over anything the call reads (cop_tx_validate's rule) or over the counters */
    cop_extent *v = (cop_extent *)malloc(((size_t)nb * 8 + 1) * sizeof(cop_extent));
    *why = "out of memory";
    if (!v) return -ENOMEM;
    uint32_t k = 0;
    cop_extent_put(v, &k, counters, ((uint64_t)cfg->rows << cfg->log2_cols) * 8, 0);
    for (uint32_t i = 0; i < nb; i++) {
        const uint64_t n = batches[i].n;
        if (!n) continue;
        cop_extent_put_batch(v, &k, &batches[i], NULL, n_lists, seg);
        cop_extent_put(v, &k, pol[i].out_idx, n * 4 * (seg ? 1u : n_lists), 1);
        cop_extent_put(v, &k, pol[i].out_count, 4ull * cop_tx_fwd_count_words(batches[i].n, n_lists, seg), 1);
        cop_extent_put(v, &k, pol[i].status, 16ull * n_lists, 1);
    }
    const int bad = cop_extents_clash(v, k, 1);
    free(v);
    *why = "an output extent overlaps a batch's packets, offsets, records or lists, or the sketch's counters";
    if (bad) return -EINVAL;
    *why = "";
    return 0;
}

/* ---- the mirror ------------------------------------------------------------ */
typedef struct {
    uint32_t a[COP_SKETCH_MAX_ROWS], b[COP_SKETCH_MAX_ROWS];
    uint32_t rows, col_shift, key_shift, dst;
    uint64_t cols;
} hashes;

static void hashes_of(const cop_sketch_config *cfg, hashes *h)
{
    (void)cop_sketch_params(cfg, h->a, h->b);
    h->rows = cfg->rows;
    h->col_shift = 32 - cfg->log2_cols;
    h->key_shift = 32 - cfg->key_depth;
    h->dst = cfg->key == COP_SKETCH_KEY_DST;
    h->cols = 1ull << cfg->log2_cols;
}

static uint64_t est_of(const hashes *h, const uint64_t *ctr, uint32_t k)
{
    uint64_t e = UINT64_MAX;
    for (uint32_t r = 0; r < h->rows; r++) {
        const uint64_t v = ctr[r * h->cols + ((uint32_t)(k * h->a[r] + h->b[r]) >> h->col_shift)];
        if (v < e) e = v;
    }
    return e;
}

static uint32_t be32(const uint8_t *p)
{
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

/* packet i of the batch: 1 and *key if it counts as IPv4, else 0 */
static int packet_key(const cop_batch *b, const hashes *h, uint32_t i, uint32_t *key)
{
    const uint8_t *p =
        (const uint8_t *)b->pkts + (b->offsets ? (uint64_t)b->offsets[i] : (uint64_t)i * b->stride) + b->data_off;
    const uint8_t *et, *ad;
    if (!b->offsets && b->stride == COP_HDR16_STRIDE) {
        et = p;        /* record bytes 0..3 = frame bytes 12..15 */
        ad = p + 6;    /* 6..9 src, 10..13 dst */
    } else {
        et = p + 12;
        ad = p + 26;
    }
    if (et[0] != 0x08 || et[1] != 0x00 || (et[2] >> 4) != 4) return 0;
    *key = be32(ad + (h->dst ? 4 : 0)) >> h->key_shift;
    return 1;
}

int cop_sketch_update_host(const cop_sketch_config *cfg, uint64_t *counters, const cop_batch *batches, uint32_t nb,
                           uint32_t verdict_mask, uint32_t max_batch)
{
    if (cop_sketch_config_check(cfg, NULL) || !counters) return -EINVAL;
    if (nb == 0) return 0;
    if (cop_sketch_update_validate(batches, nb, verdict_mask, max_batch, NULL)) return -EINVAL;
    hashes h;
    hashes_of(cfg, &h);
    for (uint32_t j = 0; j < nb; j++) {
        const cop_batch *b = &batches[j];
        for (uint32_t i = 0; i < b->n; i++) {
            uint32_t k;
            if (verdict_mask && !((verdict_mask >> b->results[i].verdict) & 1u)) continue;
            if (!packet_key(b, &h, i, &k)) continue;
            for (uint32_t r = 0; r < h.rows; r++)
                counters[r * h.cols + ((uint32_t)(k * h.a[r] + h.b[r]) >> h.col_shift)]++;
        }
    }
    return 0;
}

int cop_sketch_query_host(const cop_sketch_config *cfg, const uint64_t *counters, const uint32_t *ips, uint32_t n,
                          uint64_t *out)
{
    if (cop_sketch_query_validate(cfg, counters, ips, n, out, NULL)) return -EINVAL;
    hashes h;
    hashes_of(cfg, &h);
    for (uint32_t i = 0; i < n; i++) out[i] = est_of(&h, counters, ips[i] >> h.key_shift);
    return 0;
}

/* one chunk of a list: cnt entries at idx, the kept ones to out; returns their number */
static uint32_t police_chunk(const cop_batch *b, const hashes *h, const uint64_t *ctr, uint64_t threshold,
                             const uint32_t *idx, uint32_t cnt, uint32_t *out)
{
    uint32_t kept = 0;
    for (uint32_t j = 0; j < cnt; j++) {
        const uint32_t e = idx[j], i = e < b->n ? e : b->n - 1;
        uint32_t k;
        if (!packet_key(b, h, i, &k) || est_of(h, ctr, k) < threshold) out[kept++] = e;
    }
    return kept;
}

int cop_sketch_police_host(const cop_sketch_config *cfg, const uint64_t *counters, const cop_batch *batches,
                           const cop_police_desc *pol, uint32_t nb, uint32_t n_lists, int seg, uint32_t max_batch)
{
    if (cop_sketch_config_check(cfg, NULL) || !counters) return -EINVAL;
    if (nb == 0) return 0;
    if (cop_sketch_police_validate(cfg, counters, batches, pol, nb, n_lists, seg, max_batch, NULL)) return -EINVAL;
    hashes h;
    hashes_of(cfg, &h);
    for (uint32_t j = 0; j < nb; j++) {
        const cop_batch *b = &batches[j];
        const cop_police_desc *p = &pol[j];
        const uint32_t n = b->n;
        if (!n) continue;
        if (seg) {
            uint32_t kept = 0, total = 0;
            for (uint32_t s = 0; s * COP_SEG_PKTS < n; s++) {
                const uint32_t cap = n - s * COP_SEG_PKTS < COP_SEG_PKTS ? n - s * COP_SEG_PKTS : COP_SEG_PKTS;
                const uint32_t cnt = b->fwd_count[s] < cap ? b->fwd_count[s] : cap;
                const uint32_t k = police_chunk(b, &h, counters, p->threshold, b->fwd_idx + (size_t)s * COP_SEG_PKTS,
                                                cnt, p->out_idx + (size_t)s * COP_SEG_PKTS);
                p->out_count[s] = k;
                kept += k;
                total += cnt;
            }
            p->status[0] = kept;
            p->status[1] = total - kept;
            p->status[2] = p->status[3] = 0;
            continue;
        }
        for (uint32_t q = 0; q < n_lists; q++) {
            const uint32_t total = b->fwd_count[q] < n ? b->fwd_count[q] : n;
            uint32_t kept = 0;
            for (uint32_t c0 = 0; c0 < total; c0 += COP_SEG_PKTS) {
                const uint32_t cnt = total - c0 < COP_SEG_PKTS ? total - c0 : COP_SEG_PKTS;
                kept += police_chunk(b, &h, counters, p->threshold, b->fwd_idx + (size_t)q * n + c0, cnt,
                                     p->out_idx + (size_t)q * n + kept);
            }
            p->out_count[q] = kept;
            p->status[4 * q + 0] = kept;
            p->status[4 * q + 1] = total - kept;
            p->status[4 * q + 2] = p->status[4 * q + 3] = 0;
        }
    }
    return 0;
}
