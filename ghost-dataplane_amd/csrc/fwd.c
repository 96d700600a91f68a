/*
 * fwd.c — cop_fwd_check_host / cop_fwd_rewrite_host / cop_ipv4_csum_host: the
 * L3 forward step over host memory, the mirror of the device kernels
 * (cop_fwd.hip), and the argument checks both share (include/cop_gpu.h "L3
 * forward").
 *
 * The mirror walks every list the way the kernels cut it up: in chunks of
 * COP_SEG_PKTS positions (a segment; positions 256c .. of a dense or
 * per-vport list). It writes what the kernels write and nothing else.
 */
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "cop_internal.h"

static int common_check(const void *entries, uint32_t n_entries, const cop_fwd_config *cfg, uint32_t n_lists, int seg,
                        const char **why)
{
    *why = "null table or config";
    if (!entries || !cfg) return -EINVAL;
    *why = "n_entries must be 1 .. 1 << 24";
    if (n_entries < 1 || n_entries > (1u << 24)) return -EINVAL;
    *why = "unknown cfg.flags";
    if (cfg->flags & ~COP_FWD_VERIFY_CSUM) return -EINVAL;
    *why = "list layout: 1..COP_MAX_DEMUX_PORTS lists per batch, segmented lists one";
    if (n_lists < 1 || n_lists > COP_MAX_DEMUX_PORTS || (seg && n_lists != 1)) return -EINVAL;
    return 0;
}

/* what both calls read of a batch */
static int batch_check(const cop_batch *b, uint32_t max_batch, const char **why)
{
    *why = "n > max_batch or n > 1 << 28";
    if ((max_batch && b->n > max_batch) || b->n > (1u << 28)) return -EINVAL;
    if (cop_batch_lists_check(b, why)) return -EINVAL;
    *why = "a slot batch's stride must be at least 48 (header records are not taken)";
    if (!b->offsets && b->n && b->stride < 48) return -EINVAL;
    *why = "offsets / fwd_idx / fwd_count must be 4-byte aligned, results 8-byte aligned";
    if ((((uintptr_t)b->offsets | (uintptr_t)b->fwd_idx | (uintptr_t)b->fwd_count) & 3) || ((uintptr_t)b->results & 7))
        return -EINVAL;
    return 0;
}

int cop_fwd_check_validate(const void *entries, uint32_t n_entries, const cop_fwd_config *cfg, const cop_batch *batches,
                           const cop_fwd_check_desc *desc, uint32_t nb, uint32_t n_lists, int seg, uint32_t max_batch,
                           const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    if (common_check(entries, n_entries, cfg, n_lists, seg, why)) return -EINVAL;
    *why = "null argument";
    if (nb && (!batches || !desc)) return -EINVAL;
    for (uint32_t i = 0; i < nb; i++) {
        const cop_batch *b = &batches[i];
        const cop_fwd_check_desc *d = &desc[i];
        if (batch_check(b, max_batch, why)) return -EINVAL;
        *why = "a batch with packets needs out_idx, out_count and status";
        if (b->n && (!d->out_idx || !d->out_count || !d->status)) return -EINVAL;
        *why = "exc_idx and exc_count: both or neither";
        if (!d->exc_idx != !d->exc_count) return -EINVAL;
        *why = "an IMIX batch needs lens, a slot batch takes none";
        if (b->offsets ? (b->n && !d->lens) : d->lens != NULL) return -EINVAL;
        *why = "lens / out_idx / out_count / exc_idx / exc_count must be 4-byte aligned, status 16-byte aligned";
        if ((((uintptr_t)d->lens | (uintptr_t)d->out_idx | (uintptr_t)d->out_count | (uintptr_t)d->exc_idx |
              (uintptr_t)d->exc_count) & 3) || ((uintptr_t)d->status & 15))
            return -EINVAL;
    }
    cop_extent *v = (cop_extent *)malloc(((size_t)nb * 11 + 1) * sizeof(cop_extent));
    *why = "out of memory";
    if (!v) return -ENOMEM;
    uint32_t k = 0;
    cop_extent_put(v, &k, entries, 16ull * n_entries, 0);
    for (uint32_t i = 0; i < nb; i++) {
        const cop_batch *b = &batches[i];
        const cop_fwd_check_desc *d = &desc[i];
        const uint64_t n = b->n, idx_bytes = n * 4 * (seg ? 1u : n_lists),
                       cnt_bytes = 4ull * cop_tx_fwd_count_words(b->n, n_lists, seg);
        if (!n) continue;
        cop_extent_put_batch(v, &k, b, d->lens, n_lists, seg);
        cop_extent_put(v, &k, d->out_idx, idx_bytes, 1);
        cop_extent_put(v, &k, d->out_count, cnt_bytes, 1);
        cop_extent_put(v, &k, d->exc_idx, idx_bytes, 1);
        cop_extent_put(v, &k, d->exc_count, cnt_bytes, 1);
        cop_extent_put(v, &k, d->status, 16ull * n_lists, 1);
    }
    const int bad = cop_extents_clash(v, k, 0);
    free(v);
    *why = "an output extent overlaps another extent of the call or the table";
    if (bad) return -EINVAL;
    *why = "";
    return 0;
}

int cop_fwd_rewrite_validate(const void *entries, uint32_t n_entries, const cop_fwd_config *cfg,
                             const cop_batch *batches, const cop_tx_desc *tx, const cop_fwd_rw_desc *rw, uint32_t nb,
                             uint32_t n_lists, int seg, uint32_t max_batch, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    if (common_check(entries, n_entries, cfg, n_lists, seg, why)) return -EINVAL;
    *why = "null argument";
    if (nb && (!batches || !tx || !rw)) return -EINVAL;
    const int trc = cop_tx_validate(batches, tx, nb, n_lists, seg, max_batch, why);
    if (trc) return trc;
    for (uint32_t i = 0; i < nb; i++) {
        const cop_batch *b = &batches[i];
        if (batch_check(b, max_batch, why)) return -EINVAL;
        *why = "a slot batch needs copy_bytes >= 48";
        if (!b->offsets && tx[i].copy_bytes < 48) return -EINVAL;
        for (uint32_t q = 0; q < n_lists; q++) {
            *why = "an IMIX burst needs off and len";
            if (b->offsets && (!tx[i].out[q].off || !tx[i].out[q].len)) return -EINVAL;
            *why = "status must be non-NULL and 16-byte aligned, port 4-byte aligned";
            if ((b->n && !rw[i].status[q]) || ((uintptr_t)rw[i].status[q] & 15) || ((uintptr_t)rw[i].port[q] & 3))
                return -EINVAL;
        }
    }
    cop_extent *v = (cop_extent *)malloc(((size_t)nb * (3 + 6 * COP_MAX_DEMUX_PORTS) + 1) * sizeof(cop_extent));
    *why = "out of memory";
    if (!v) return -ENOMEM;
    uint32_t k = 0;
    cop_extent_put(v, &k, entries, 16ull * n_entries, 0);
    for (uint32_t i = 0; i < nb; i++) {
        const cop_batch *b = &batches[i];
        const uint64_t n = b->n;
        if (!n) continue;
        cop_extent_put(v, &k, b->results, n * 8, 0);
        cop_extent_put(v, &k, b->fwd_idx, n * 4 * (seg ? 1u : n_lists), 0);
        cop_extent_put(v, &k, b->fwd_count, 4ull * cop_tx_fwd_count_words(b->n, n_lists, seg), 0);
        for (uint32_t q = 0; q < n_lists; q++) {
            const cop_tx_burst *o = &tx[i].out[q];
            cop_extent_put(v, &k, o->frames, o->cap_bytes, 1);
            cop_extent_put(v, &k, o->off, 4ull * o->cap_frames, 0);
            cop_extent_put(v, &k, o->len, 4ull * o->cap_frames, 0);
            cop_extent_put(v, &k, o->status, 16, 0);
            cop_extent_put(v, &k, rw[i].port[q], 4ull * o->cap_frames, 1);
            cop_extent_put(v, &k, rw[i].status[q], 16, 1);
        }
    }
    const int bad = cop_extents_clash(v, k, 0);
    free(v);
    *why = "an output extent overlaps another extent of the call or the table";
    if (bad) return -EINVAL;
    *why = "";
    return 0;
}

/* ---- the mirror ------------------------------------------------------------ */
static uint32_t fold16(uint32_t v)
{
    while (v >> 16) v = (v & 0xFFFFu) + (v >> 16);
    return v;
}

uint16_t cop_ipv4_csum_host(const uint8_t hdr[20])
{
    uint32_t s = 0;
    for (int j = 0; j < 10; j++)
        if (j != 5) s += ((uint32_t)hdr[2 * j] << 8) | hdr[2 * j + 1];
    return (uint16_t)(~fold16(s) & 0xFFFFu);
}

typedef struct {
    const cop_neigh_entry *tab;
    uint32_t n_entries, verify, miss_nh;
} fwd_tab;

/* the class of frame b (is_short: nothing of it is read); *ent the entry of an OK frame */
static uint32_t class_of(const fwd_tab *t, const uint8_t *b, int is_short, const cop_result *r,
                         const cop_neigh_entry **ent)
{
    if (is_short) return COP_FWD_SHORT;
    if (b[12] != 0x08 || b[13] != 0x00 || (b[14] >> 4) != 4) return COP_FWD_PASS;
    const uint32_t ihl = b[14] & 15u;
    if (ihl < 5) return COP_FWD_BAD_HDR;
    if (ihl > 5) return COP_FWD_OPTIONS;
    if (t->verify) {
        uint32_t s = 0;
        for (int j = 0; j < 10; j++) s += ((uint32_t)b[14 + 2 * j] << 8) | b[15 + 2 * j];
        if (fold16(s) != 0xFFFFu) return COP_FWD_BAD_CSUM;
    }
    if (b[22] <= 1) return COP_FWD_TTL;
    const uint32_t nh = (r && (r->flags & COP_FLAG_ROUTE_HIT)) ? (r->route_nh & 0xFFFFFFu) : t->miss_nh;
    if (nh >= t->n_entries || !(t->tab[nh].flags & COP_NEIGH_VALID)) return COP_FWD_NO_NEIGH;
    *ent = &t->tab[nh];
    return COP_FWD_OK;
}

typedef struct {
    uint32_t kept, removed, ttl, no_neigh;
} tally;

/* one chunk of a list: cnt entries at idx, the kept ones to out, the removed ones to exc (or NULL) */
static void check_chunk(const fwd_tab *t, const cop_batch *b, const uint32_t *lens, const uint32_t *idx, uint32_t cnt,
                        uint32_t *out, uint32_t *exc, tally *y)
{
    uint32_t kept = 0, removed = 0;
    for (uint32_t j = 0; j < cnt; j++) {
        const uint32_t e = idx[j], i = e < b->n ? e : b->n - 1;
        const uint8_t *p =
            (const uint8_t *)b->pkts + (b->offsets ? (uint64_t)b->offsets[i] : (uint64_t)i * b->stride) + b->data_off;
        int is_short = 0;
        if (b->offsets) {
            const uint32_t l = lens[i] < 1 ? 1 : lens[i] > COP_TX_MAX_FRAME ? COP_TX_MAX_FRAME : lens[i];
            is_short = l < 34;
        }
        const cop_neigh_entry *ent;
        const uint32_t cls = class_of(t, p, is_short, b->results ? &b->results[i] : NULL, &ent);
        if (cls == COP_FWD_OK || cls == COP_FWD_PASS) {
            out[kept++] = e;
            continue;
        }
        if (exc) exc[removed] = i | (cls << 28);
        removed++;
        y->ttl += cls == COP_FWD_TTL;
        y->no_neigh += cls == COP_FWD_NO_NEIGH;
    }
    y->kept += kept;
    y->removed += removed;
}

static fwd_tab tab_of(const cop_neigh_entry *entries, uint32_t n_entries, const cop_fwd_config *cfg)
{
    fwd_tab t = {entries, n_entries, cfg->flags & COP_FWD_VERIFY_CSUM, cfg->miss_nh};
    return t;
}

int cop_fwd_check_host(const cop_neigh_entry *entries, uint32_t n_entries, const cop_fwd_config *cfg,
                       const cop_batch *batches, const cop_fwd_check_desc *desc, uint32_t nb, uint32_t n_lists,
                       int seg, uint32_t max_batch)
{
    if (nb == 0) return entries && cfg ? 0 : -EINVAL;
    const int rc = cop_fwd_check_validate(entries, n_entries, cfg, batches, desc, nb, n_lists, seg, max_batch, NULL);
    if (rc) return rc;
    const fwd_tab t = tab_of(entries, n_entries, cfg);
    for (uint32_t j = 0; j < nb; j++) {
        const cop_batch *b = &batches[j];
        const cop_fwd_check_desc *d = &desc[j];
        const uint32_t n = b->n;
        if (!n) continue;
        if (seg) {
            tally y = {0, 0, 0, 0};
            for (uint32_t s = 0; s * COP_SEG_PKTS < n; s++) {
                const uint32_t cap = n - s * COP_SEG_PKTS < COP_SEG_PKTS ? n - s * COP_SEG_PKTS : COP_SEG_PKTS;
                const uint32_t cnt = b->fwd_count[s] < cap ? b->fwd_count[s] : cap;
                const tally was = y;
                check_chunk(&t, b, d->lens, b->fwd_idx + (size_t)s * COP_SEG_PKTS, cnt,
                            d->out_idx + (size_t)s * COP_SEG_PKTS,
                            d->exc_idx ? d->exc_idx + (size_t)s * COP_SEG_PKTS : NULL, &y);
                d->out_count[s] = y.kept - was.kept;
                if (d->exc_count) d->exc_count[s] = y.removed - was.removed;
            }
            d->status[0] = y.kept, d->status[1] = y.removed, d->status[2] = y.ttl, d->status[3] = y.no_neigh;
            continue;
        }
        for (uint32_t q = 0; q < n_lists; q++) {
            const uint32_t total = b->fwd_count[q] < n ? b->fwd_count[q] : n;
            tally y = {0, 0, 0, 0};
            for (uint32_t c0 = 0; c0 < total; c0 += COP_SEG_PKTS) {
                const uint32_t cnt = total - c0 < COP_SEG_PKTS ? total - c0 : COP_SEG_PKTS;
                check_chunk(&t, b, d->lens, b->fwd_idx + (size_t)q * n + c0, cnt, d->out_idx + (size_t)q * n + y.kept,
                            d->exc_idx ? d->exc_idx + (size_t)q * n + y.removed : NULL, &y);
            }
            d->out_count[q] = y.kept;
            if (d->exc_count) d->exc_count[q] = y.removed;
            uint32_t *st = d->status + 4 * q;
            st[0] = y.kept, st[1] = y.removed, st[2] = y.ttl, st[3] = y.no_neigh;
        }
    }
    return 0;
}

/* frame k of a burst, the frame of list entry e */
static void rewrite_frame(const fwd_tab *t, const cop_batch *b, const cop_tx_burst *o, uint32_t slot_bytes, uint32_t k,
                          uint32_t e, uint32_t *port, uint32_t st[3])
{
    const uint32_t i = e < b->n ? e : b->n - 1;
    const uint64_t at = b->offsets ? (uint64_t)o->off[k] : (uint64_t)k * slot_bytes;
    int is_short = (at & 15) || at + 48 > o->cap_bytes;
    if (b->offsets && o->len[k] < 34) is_short = 1;
    uint8_t *f = (uint8_t *)o->frames + at;
    const cop_neigh_entry *ent = NULL;
    const uint32_t cls = class_of(t, f, is_short, b->results ? &b->results[i] : NULL, &ent);
    if (port) port[k] = cls == COP_FWD_OK ? ent->port : 0xFFFFu;
    st[cls == COP_FWD_OK ? 0 : cls == COP_FWD_PASS ? 1 : 2]++;
    if (cls != COP_FWD_OK) return;
    const uint32_t m = ((uint32_t)f[22] << 8) | f[23], m2 = m - 0x0100u, hc = ((uint32_t)f[24] << 8) | f[25];
    const uint32_t hc2 = ~fold16((~hc & 0xFFFFu) + (~m & 0xFFFFu) + m2) & 0xFFFFu;
    memcpy(f, ent->dst_mac, 6);
    memcpy(f + 6, ent->src_mac, 6);
    f[22] = (uint8_t)(f[22] - 1);
    f[24] = (uint8_t)(hc2 >> 8);
    f[25] = (uint8_t)hc2;
}

int cop_fwd_rewrite_host(const cop_neigh_entry *entries, uint32_t n_entries, const cop_fwd_config *cfg,
                         const cop_batch *batches, const cop_tx_desc *tx, const cop_fwd_rw_desc *rw, uint32_t nb,
                         uint32_t n_lists, int seg, uint32_t max_batch)
{
    if (nb == 0) return entries && cfg ? 0 : -EINVAL;
    const int rc = cop_fwd_rewrite_validate(entries, n_entries, cfg, batches, tx, rw, nb, n_lists, seg, max_batch, NULL);
    if (rc) return rc;
    const fwd_tab t = tab_of(entries, n_entries, cfg);
    for (uint32_t j = 0; j < nb; j++) {
        const cop_batch *b = &batches[j];
        const uint32_t n = b->n;
        if (!n) continue;
        for (uint32_t q = 0; q < n_lists; q++) {
            const cop_tx_burst *o = &tx[j].out[q];
            uint32_t st[3] = {0, 0, 0}, k = 0;
            uint32_t W = o->status[0] < o->cap_frames ? o->status[0] : o->cap_frames;
            const uint32_t nchunk = seg ? (n + COP_SEG_PKTS - 1) / COP_SEG_PKTS : 1;
            for (uint32_t s = 0; s < nchunk && k < W; s++) {
                uint32_t cnt;
                if (seg) {
                    const uint32_t cap = n - s * COP_SEG_PKTS < COP_SEG_PKTS ? n - s * COP_SEG_PKTS : COP_SEG_PKTS;
                    cnt = b->fwd_count[s] < cap ? b->fwd_count[s] : cap;
                } else {
                    cnt = b->fwd_count[q] < n ? b->fwd_count[q] : n;
                }
                const uint32_t *idx = b->fwd_idx + (seg ? (size_t)s * COP_SEG_PKTS : (size_t)q * n);
                for (uint32_t x = 0; x < cnt && k < W; x++, k++)
                    rewrite_frame(&t, b, o, tx[j].slot_bytes, k, idx[x], rw[j].port[q], st);
            }
            uint32_t *out = rw[j].status[q];
            out[0] = st[0], out[1] = st[1], out[2] = st[2], out[3] = 0;
        }
    }
    return 0;
}
