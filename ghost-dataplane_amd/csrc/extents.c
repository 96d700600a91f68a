/*
 * extents.c — what the side calls' argument checks share (tx_gather.c,
 * sketch.c, aead.c, fwd.c; declared in cop_internal.h): the overlap rules over
 * the memory extents of a call, the fwd_count layout, and the batch checks.
 *
 * A validator lists every extent its call reads or writes and asks one of two
 * questions. Both sort the extents by start and sweep once: an extent meets
 * an earlier one iff it starts below the largest end so far, kept apart for
 * the written and the read extents. Microseconds for 32 batches.
 */
#include <errno.h>

#include "cop_internal.h"

void cop_extent_put(cop_extent *v, uint32_t *k, const void *p, uint64_t bytes, int written)
{
    if (!p || !bytes) return;
    v[*k].start = (uintptr_t)p;
    v[*k].end = (uintptr_t)p + bytes;
    v[*k].written = written;
    (*k)++;
}

/* by start; a Shell sort (gaps 3h + 1), in place and with the comparison inline: the validators run
 * on every side call, and qsort's indirect calls cost a call's few hundred extents several microseconds */
static void sort_by_start(cop_extent *v, uint32_t k)
{
    uint32_t g = 1;
    while (g < k / 3) g = 3 * g + 1;
    for (; g; g /= 3)
        for (uint32_t i = g; i < k; i++) {
            const cop_extent x = v[i];
            uint32_t j = i;
            for (; j >= g && v[j - g].start > x.start; j -= g) v[j] = v[j - g];
            v[j] = x;
        }
}

int cop_extents_clash(cop_extent *v, uint32_t k, int outputs_may_meet)
{
    sort_by_start(v, k);
    uintptr_t end_r = 0, end_w = 0;
    for (uint32_t i = 0; i < k; i++) {
        if (v[i].start < (v[i].written ? end_r : end_w)) return 1;
        if (v[i].written) {
            if (!outputs_may_meet && v[i].start < end_w) return 1;
            if (v[i].end > end_w) end_w = v[i].end;
        } else if (v[i].end > end_r) {
            end_r = v[i].end;
        }
    }
    return 0;
}

uint32_t cop_tx_fwd_count_words(uint32_t n, uint32_t n_lists, int seg)
{
    return seg ? (n + COP_SEG_PKTS - 1) / COP_SEG_PKTS : n_lists;
}

void cop_extent_put_batch(cop_extent *v, uint32_t *k, const cop_batch *b, const uint32_t *lens, uint32_t n_lists, int seg)
{
    const uint64_t n = b->n;
    /* an IMIX slab's size is not known here: its first byte stands for it */
    cop_extent_put(v, k, b->pkts, b->offsets ? 16 : n * b->stride, 0);
    cop_extent_put(v, k, b->offsets, n * 4, 0);
    cop_extent_put(v, k, lens, n * 4, 0);
    cop_extent_put(v, k, b->results, n * 8, 0);
    cop_extent_put(v, k, b->fwd_idx, n * 4 * (seg ? 1u : n_lists), 0);
    cop_extent_put(v, k, b->fwd_count, 4ull * cop_tx_fwd_count_words(b->n, n_lists, seg), 0);
}

int cop_batch_misaligned(const cop_batch *b)
{
    return ((uintptr_t)b->pkts & 15) || (b->data_off & 15) || (!b->offsets && (b->stride & 15));
}

int cop_batch_lists_check(const cop_batch *b, const char **why)
{
    *why = "a batch with packets needs pkts, fwd_idx and fwd_count";
    if (b->n && (!b->pkts || !b->fwd_idx || !b->fwd_count)) return -EINVAL;
    *why = "packet starts must be 16-byte aligned (pkts, data_off, stride)";
    if (cop_batch_misaligned(b)) return -EINVAL;
    return 0;
}
