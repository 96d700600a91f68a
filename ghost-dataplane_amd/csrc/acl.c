/*
 * acl.c — cop_acl_build and the cop_acl_*_host mirror of the device kernels
 * (cop_acl.hip), and the argument checks both share (include/cop_gpu.h "ACL").
 *
 * The image is a bit-vector classifier. Rules are ranked by (priority
 * descending, index ascending); rank p is bit p of a row of row_words u32
 * (bit p of the row: word p / 32, bit p % 32). Each of the four range fields
 * (src, dst, sport, dport; a prefix is a range) cuts its key space at every
 * rule's lo and hi + 1 into at most 2n + 1 intervals, kept as a sorted array
 * of starts (starts[0] == 0) with one row per interval: bit p set iff rule p
 * covers the interval. The protocol has 256 rows, indexed directly. A key's
 * word: the AND of its five rows, the first set bit, the rank table's word of
 * that rank; no bit: 0. One array of u32 holds all of it, every part at a
 * multiple of four words, so a row is 16-byte aligned wherever the array is.
 *
 * The filter mirror walks every list the way the kernels cut it up, in chunks
 * of COP_SEG_PKTS positions, and writes what they write and nothing else.
 */
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "cop_internal.h"

static uint32_t pad4(uint32_t w) { return (w + 3u) & ~3u; }

/* rule r's inclusive range of field f (0 src, 1 dst, 2 sport, 3 dport) */
static void rule_range(const cop_acl_rule *r, int f, uint32_t *lo, uint32_t *hi)
{
    if (f < 2) {
        const uint32_t ip = f ? r->dst_ip : r->src_ip, depth = f ? r->dst_depth : r->src_depth;
        const uint32_t mask = depth ? 0xFFFFFFFFu << (32 - depth) : 0u;
        *lo = ip & mask;
        *hi = *lo | ~mask;
    } else {
        *lo = f == 2 ? r->sport_lo : r->dport_lo;
        *hi = f == 2 ? r->sport_hi : r->dport_hi;
    }
}

static int cmp_u32(const void *a, const void *b)
{
    const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
    return x < y ? -1 : x > y;
}

/* the interval of key k: the last j with starts[j] <= k (starts[0] == 0); at most 12 steps for 2049 */
static uint32_t interval_of(const uint32_t *starts, uint32_t niv, uint32_t k)
{
    uint32_t lo = 0, hi = niv;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (starts[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}

typedef struct {
    int32_t priority;
    uint32_t idx;
} ranked;

static int cmp_ranked(const void *a, const void *b)
{
    const ranked *x = (const ranked *)a, *y = (const ranked *)b;
    if (x->priority != y->priority) return x->priority > y->priority ? -1 : 1;
    return x->idx < y->idx ? -1 : x->idx > y->idx;
}

int cop_acl_build(const cop_acl_rule *rules, uint32_t n, cop_acl_table **out, cop_acl_report *rep)
{
    if (rep) {
        memset(rep, 0, sizeof(*rep));
        rep->first_error_idx = 0xFFFFFFFFu;
    }
    if (!out || (n && !rules)) return -EINVAL;
    *out = NULL;
    if (n > COP_ACL_MAX_RULES) {
        if (rep) rep->first_error_idx = n;
        return -ENOSPC;
    }
    for (uint32_t i = 0; i < n; i++) {
        const cop_acl_rule *r = &rules[i];
        if (r->src_depth > 32 || r->dst_depth > 32 || r->sport_lo > r->sport_hi || r->dport_lo > r->dport_hi) {
            if (rep) rep->first_error_idx = i;
            return -EINVAL;
        }
    }
    cop_acl_table *t = (cop_acl_table *)calloc(1, sizeof(*t));
    ranked *rk = (ranked *)malloc(((size_t)n + 1) * sizeof(ranked));
    uint32_t *cut = (uint32_t *)malloc((2 * (size_t)n + 1) * sizeof(uint32_t));
    uint32_t *starts[4] = {NULL, NULL, NULL, NULL};
    int rc = -ENOMEM;
    if (!t || !rk || !cut) goto fail;
    for (uint32_t i = 0; i < n; i++) {
        rk[i].priority = rules[i].priority;
        rk[i].idx = i;
    }
    qsort(rk, n, sizeof(ranked), cmp_ranked);

    cop_acl_layout *L = &t->lay;
    L->n_rules = n;
    L->row_words = 4u * (((n ? n : 1u) + 127u) / 128u);
    uint32_t at = 0;
    for (int f = 0; f < 4; f++) {
        const uint64_t top = f < 2 ? 0xFFFFFFFFull : 0xFFFFull;
        uint32_t k = 0;
        cut[k++] = 0;
        for (uint32_t i = 0; i < n; i++) {
            uint32_t lo, hi;
            rule_range(&rules[i], f, &lo, &hi);
            cut[k++] = lo;
            if (hi < top) cut[k++] = hi + 1u;
        }
        qsort(cut, k, sizeof(uint32_t), cmp_u32);
        uint32_t m = 0;
        for (uint32_t i = 0; i < k; i++)
            if (!m || cut[i] != cut[m - 1]) cut[m++] = cut[i];
        starts[f] = (uint32_t *)malloc((size_t)m * sizeof(uint32_t));
        if (!starts[f]) goto fail;
        memcpy(starts[f], cut, (size_t)m * sizeof(uint32_t));
        L->niv[f] = m;
        L->off_starts[f] = at;
        at += pad4(m);
        L->off_rows[f] = at;
        at += m * L->row_words;
    }
    L->off_proto = at;
    at += 256u * L->row_words;
    L->off_rank = at;
    at += pad4(n ? n : 1u);
    L->words = at;
    t->image = (uint32_t *)calloc(at, sizeof(uint32_t));
    if (!t->image) goto fail;

    for (int f = 0; f < 4; f++) {
        uint32_t *const s = t->image + L->off_starts[f];
        memcpy(s, starts[f], (size_t)L->niv[f] * sizeof(uint32_t));
        for (uint32_t j = L->niv[f]; j < pad4(L->niv[f]); j++) s[j] = 0xFFFFFFFFu;   /* never searched */
        for (uint32_t p = 0; p < n; p++) {
            uint32_t lo, hi;
            rule_range(&rules[rk[p].idx], f, &lo, &hi);
            /* lo and hi + 1 are starts, so the rule covers whole intervals */
            const uint32_t a = interval_of(s, L->niv[f], lo), b = interval_of(s, L->niv[f], hi);
            for (uint32_t j = a; j <= b; j++)
                t->image[L->off_rows[f] + (size_t)j * L->row_words + (p >> 5)] |= 1u << (p & 31u);
        }
    }
    for (uint32_t p = 0; p < n; p++) {
        const cop_acl_rule *r = &rules[rk[p].idx];
        for (uint32_t v = 0; v < 256; v++)
            if (((v ^ r->proto) & r->proto_mask) == 0)
                t->image[L->off_proto + (size_t)v * L->row_words + (p >> 5)] |= 1u << (p & 31u);
        t->image[L->off_rank + p] = rk[p].idx | COP_ACL_HIT | (r->action ? COP_ACL_DROP : 0u);
    }
    if (rep) {
        rep->n_rules = n;
        for (int f = 0; f < 4; f++) rep->n_intervals[f] = L->niv[f];
        rep->row_words = L->row_words;
        rep->image_bytes = (uint64_t)L->words * 4;
    }
    for (int f = 0; f < 4; f++) free(starts[f]);
    free(cut);
    free(rk);
    *out = t;
    return 0;
fail:
    for (int f = 0; f < 4; f++) free(starts[f]);
    free(cut);
    free(rk);
    if (t) free(t->image);
    free(t);
    return rc;
}

void cop_acl_free(cop_acl_table *t)
{
    if (!t) return;
    free(t->image);
    free(t);
}

static uint32_t word_of(const cop_acl_table *t, const cop_acl_key *k)
{
    const cop_acl_layout *L = &t->lay;
    const uint32_t key[4] = {k->src, k->dst, k->sport, k->dport};
    const uint32_t *row[5];
    for (int f = 0; f < 4; f++)
        row[f] = t->image + L->off_rows[f] +
                 (size_t)interval_of(t->image + L->off_starts[f], L->niv[f], key[f]) * L->row_words;
    row[4] = t->image + L->off_proto + (size_t)k->proto * L->row_words;
    for (uint32_t w = 0; w < L->row_words; w++) {
        const uint32_t x = row[0][w] & row[1][w] & row[2][w] & row[3][w] & row[4][w];
        if (x) return t->image[L->off_rank + 32u * w + (uint32_t)__builtin_ctz(x)];
    }
    return 0;
}

int cop_acl_match_host(const cop_acl_table *t, const cop_acl_key *keys, uint32_t n, uint32_t *out)
{
    if (!t || (n && (!keys || !out))) return -EINVAL;
    for (uint32_t i = 0; i < n; i++) out[i] = word_of(t, &keys[i]);
    return 0;
}

/* ---- the argument checks --------------------------------------------------- */
static int batch_packets_check(const cop_batch *b, uint32_t max_batch, const char **why)
{
    *why = "n > max_batch";
    if (max_batch && b->n > max_batch) return -EINVAL;
    *why = "a batch with packets needs pkts";
    if (b->n && !b->pkts) return -EINVAL;
    *why = "packet starts must be 16-byte aligned (pkts, data_off, stride)";
    if (cop_batch_misaligned(b)) return -EINVAL;
    *why = "a slot batch's stride must be at least 48 (header records lack the protocol and the ports)";
    if (!b->offsets && b->n && b->stride < 48) return -EINVAL;
    *why = "offsets must be 4-byte aligned";
    if ((uintptr_t)b->offsets & 3) return -EINVAL;
    return 0;
}

int cop_acl_validate(const void *image, uint64_t image_bytes, const void *counters, uint32_t n_rules,
                     const cop_batch *batches, const cop_acl_desc *descs, uint32_t nb, int filter, uint32_t n_lists,
                     int seg, uint32_t max_batch, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "null argument";
    if (!image || (nb && (!batches || !descs))) return -EINVAL;
    if (filter) {
        *why = "list layout: 1..COP_MAX_DEMUX_PORTS lists per batch, segmented lists one";
        if (n_lists < 1 || n_lists > COP_MAX_DEMUX_PORTS || (seg && n_lists != 1)) return -EINVAL;
    }
    for (uint32_t i = 0; i < nb; i++) {
        const cop_batch *b = &batches[i];
        const cop_acl_desc *d = &descs[i];
        if (batch_packets_check(b, max_batch, why)) return -EINVAL;
        if (!filter) {
            *why = "a batch with packets needs words (4-byte aligned)";
            if ((b->n && !d->words) || ((uintptr_t)d->words & 3)) return -EINVAL;
            continue;
        }
        *why = "a batch with packets needs fwd_idx, fwd_count, out_idx, out_count and status";
        if (b->n && (!b->fwd_idx || !b->fwd_count || !d->out_idx || !d->out_count || !d->status)) return -EINVAL;
        *why = "fwd_idx / fwd_count / out_idx / out_count must be 4-byte aligned, status 16-byte aligned";
        if ((((uintptr_t)b->fwd_idx | (uintptr_t)b->fwd_count | (uintptr_t)d->out_idx | (uintptr_t)d->out_count) & 3) ||
            ((uintptr_t)d->status & 15))
            return -EINVAL;
    }
    cop_extent *v = (cop_extent *)malloc(((size_t)nb * 9 + 2) * sizeof(cop_extent));
    *why = "out of memory";
    if (!v) return -ENOMEM;
    uint32_t k = 0;
    cop_extent_put(v, &k, image, image_bytes, 0);
    cop_extent_put(v, &k, counters, 8ull * n_rules, filter);
    for (uint32_t i = 0; i < nb; i++) {
        const cop_batch *b = &batches[i];
        const uint64_t n = b->n;
        if (!n) continue;
        if (!filter) {
            cop_extent_put(v, &k, b->pkts, b->offsets ? 16 : n * b->stride, 0);
            cop_extent_put(v, &k, b->offsets, n * 4, 0);
            cop_extent_put(v, &k, descs[i].words, n * 4, 1);
            continue;
        }
        cop_extent_put_batch(v, &k, b, NULL, n_lists, seg);
        cop_extent_put(v, &k, descs[i].out_idx, n * 4 * (seg ? 1u : n_lists), 1);
        cop_extent_put(v, &k, descs[i].out_count, 4ull * cop_tx_fwd_count_words(b->n, n_lists, seg), 1);
        cop_extent_put(v, &k, descs[i].status, 16ull * n_lists, 1);
    }
    const int bad = cop_extents_clash(v, k, 0);
    free(v);
    *why = "an output extent overlaps another extent of the call, the ACL's image or its counters";
    if (bad) return -EINVAL;
    *why = "";
    return 0;
}

/* ---- the mirror ------------------------------------------------------------ */
/* the word of packet i of the batch */
static uint32_t packet_word(const cop_acl_table *t, const cop_batch *b, uint32_t i)
{
    const uint8_t *p =
        (const uint8_t *)b->pkts + (b->offsets ? (uint64_t)b->offsets[i] : (uint64_t)i * b->stride) + b->data_off;
    if (p[12] != 0x08 || p[13] != 0x00 || (p[14] >> 4) != 4 || (p[14] & 15) < 5) return COP_ACL_SKIP;
    cop_acl_key k;
    memset(&k, 0, sizeof(k));
    k.proto = p[23];
    k.src = ((uint32_t)p[26] << 24) | ((uint32_t)p[27] << 16) | ((uint32_t)p[28] << 8) | p[29];
    k.dst = ((uint32_t)p[30] << 24) | ((uint32_t)p[31] << 16) | ((uint32_t)p[32] << 8) | p[33];
    if ((p[14] & 15) == 5 && (((p[20] & 0x1Fu) << 8) | p[21]) == 0) {
        k.sport = (uint16_t)((p[34] << 8) | p[35]);
        k.dport = (uint16_t)((p[36] << 8) | p[37]);
    }
    return word_of(t, &k);
}

int cop_acl_classify_host(const cop_acl_table *t, const cop_batch *batches, const cop_acl_desc *descs, uint32_t nb,
                          uint32_t max_batch)
{
    if (!t) return -EINVAL;
    if (nb == 0) return 0;
    if (cop_acl_validate(t->image, (uint64_t)t->lay.words * 4, NULL, 0, batches, descs, nb, 0, 1, 0, max_batch, NULL))
        return -EINVAL;
    for (uint32_t j = 0; j < nb; j++)
        for (uint32_t i = 0; i < batches[j].n; i++) descs[j].words[i] = packet_word(t, &batches[j], i);
    return 0;
}

/* one chunk of a list: cnt entries at idx, the kept ones to out; returns their number; st: the list's status */
static uint32_t filter_chunk(const cop_acl_table *t, uint64_t *counters, const cop_batch *b, const uint32_t *idx,
                             uint32_t cnt, uint32_t *out, uint32_t st[4])
{
    uint32_t kept = 0;
    for (uint32_t j = 0; j < cnt; j++) {
        const uint32_t e = idx[j], i = e < b->n ? e : b->n - 1;
        const uint32_t w = packet_word(t, b, i);
        if (counters && (w & COP_ACL_HIT)) counters[w & 0x00FFFFFFu]++;
        if (w & COP_ACL_DROP) {
            st[1]++;
            continue;
        }
        out[kept++] = e;
        st[0]++;
        if (w == 0) st[2]++;
        if (w == COP_ACL_SKIP) st[3]++;
    }
    return kept;
}

int cop_acl_filter_host(const cop_acl_table *t, uint64_t *counters, const cop_batch *batches, const cop_acl_desc *descs,
                        uint32_t nb, uint32_t n_lists, int seg, uint32_t max_batch)
{
    if (!t) return -EINVAL;
    if (nb == 0) return 0;
    if (cop_acl_validate(t->image, (uint64_t)t->lay.words * 4, counters, t->lay.n_rules, batches, descs, nb, 1, n_lists,
                         seg, max_batch, NULL))
        return -EINVAL;
    for (uint32_t j = 0; j < nb; j++) {
        const cop_batch *b = &batches[j];
        const cop_acl_desc *d = &descs[j];
        const uint32_t n = b->n;
        if (!n) continue;
        if (seg) {
            uint32_t st[4] = {0, 0, 0, 0};
            for (uint32_t s = 0; s * COP_SEG_PKTS < n; s++) {
                const uint32_t cap = n - s * COP_SEG_PKTS < COP_SEG_PKTS ? n - s * COP_SEG_PKTS : COP_SEG_PKTS;
                const uint32_t cnt = b->fwd_count[s] < cap ? b->fwd_count[s] : cap;
                d->out_count[s] = filter_chunk(t, counters, b, b->fwd_idx + (size_t)s * COP_SEG_PKTS, cnt,
                                               d->out_idx + (size_t)s * COP_SEG_PKTS, st);
            }
            memcpy(d->status, st, sizeof(st));
            continue;
        }
        for (uint32_t q = 0; q < n_lists; q++) {
            const uint32_t total = b->fwd_count[q] < n ? b->fwd_count[q] : n;
            uint32_t st[4] = {0, 0, 0, 0};
            for (uint32_t c0 = 0; c0 < total; c0 += COP_SEG_PKTS) {
                const uint32_t cnt = total - c0 < COP_SEG_PKTS ? total - c0 : COP_SEG_PKTS;
                (void)filter_chunk(t, counters, b, b->fwd_idx + (size_t)q * n + c0, cnt,
                                   d->out_idx + (size_t)q * n + st[0], st);
            }
            d->out_count[q] = st[0];
            memcpy(d->status + 4 * q, st, sizeof(st));
        }
    }
    return 0;
}
