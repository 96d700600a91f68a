/*
 * tx_gather.c — cop_tx_gather_host: the tx gather over host memory, the mirror
 * of the device kernels (cop_tx.hip), and the argument checks both share
 * (include/cop_gpu.h "Tx gather").
 *
 * The mirror walks every list the way the kernels cut it up: in chunks of
 * COP_SEG_PKTS positions (a segment; positions 256c .. of a dense or
 * per-vport list), a chunk's byte base being the sum of the earlier chunks'
 * extents. It writes what the kernels write and nothing else.
 */
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "cop_internal.h"

int cop_tx_validate(const cop_batch *batches, const cop_tx_desc *tx, uint32_t nb, uint32_t n_lists, int seg,
                    uint32_t max_batch, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "null argument";
    if (nb && (!batches || !tx)) return -EINVAL;
    *why = "list layout: 1..COP_MAX_DEMUX_PORTS lists per batch, segmented lists one";
    if (n_lists < 1 || n_lists > COP_MAX_DEMUX_PORTS || (seg && n_lists != 1)) return -EINVAL;
    for (uint32_t i = 0; i < nb; i++) {
        const cop_batch *b = &batches[i];
        const cop_tx_desc *t = &tx[i];
        const int imix = b->offsets != NULL;
        *why = "n > max_batch";
        if (max_batch && b->n > max_batch) return -EINVAL;
        *why = "n * COP_TX_MAX_FRAME >= 2^32";
        if ((uint64_t)b->n * COP_TX_MAX_FRAME >= (1ull << 32)) return -EINVAL;
        if (cop_batch_lists_check(b, why)) return -EINVAL;
        *why = "fwd_idx / fwd_count / offsets / lens must be 4-byte aligned";
        if (((uintptr_t)b->fwd_idx | (uintptr_t)b->fwd_count | (uintptr_t)b->offsets | (uintptr_t)t->lens) & 3)
            return -EINVAL;
        if (imix) {
            *why = "IMIX batch: lens needed, copy_bytes and slot_bytes 0";
            if ((b->n && !t->lens) || t->copy_bytes || t->slot_bytes) return -EINVAL;
        } else {
            *why = "slot batch: copy_bytes a multiple of 16 in 16 .. min(stride - data_off, COP_TX_MAX_FRAME), "
                   "slot_bytes a multiple of 16 >= copy_bytes, lens NULL";
            if (t->lens || (t->copy_bytes & 15) || t->copy_bytes < 16 || t->copy_bytes > COP_TX_MAX_FRAME ||
                b->data_off > b->stride || t->copy_bytes > b->stride - b->data_off || (t->slot_bytes & 15) ||
                t->slot_bytes < t->copy_bytes)
                return -EINVAL;
        }
        for (uint32_t q = 0; q < n_lists; q++) {
            const cop_tx_burst *o = &t->out[q];
            *why = "frames and status must be non-NULL and 16-byte aligned, off / len 4-byte aligned";
            if (!o->frames || !o->status || (((uintptr_t)o->frames | (uintptr_t)o->status) & 15) ||
                (((uintptr_t)o->off | (uintptr_t)o->len) & 3))
                return -EINVAL;
            *why = "cap_bytes >= 2^32";
            if (o->cap_bytes >= (1ull << 32)) return -EINVAL;
        }
    }
    /* no output extent over anything the call reads; outputs may meet each other */
    cop_extent *v = (cop_extent *)malloc(((size_t)nb * (6 + 4 * n_lists) + 1) * sizeof(cop_extent));
    *why = "out of memory";
    if (!v) return -ENOMEM;
    uint32_t k = 0;
    for (uint32_t i = 0; i < nb; i++) {
        if (batches[i].n) cop_extent_put_batch(v, &k, &batches[i], tx[i].lens, n_lists, seg);
        for (uint32_t q = 0; q < n_lists; q++) {
            const cop_tx_burst *o = &tx[i].out[q];
            cop_extent_put(v, &k, o->frames, o->cap_bytes, 1);
            cop_extent_put(v, &k, o->off, 4ull * o->cap_frames, 1);
            cop_extent_put(v, &k, o->len, 4ull * o->cap_frames, 1);
            cop_extent_put(v, &k, o->status, 16, 1);
        }
    }
    const int bad = cop_extents_clash(v, k, 1);
    free(v);
    *why = "an output extent overlaps a batch's packets, offsets, lens, records or lists";
    if (bad) return -EINVAL;
    *why = "";
    return 0;
}

/* one list: positions [0, count) cut into chunks by chunk_of (dense lists:
 * 256 positions; segmented: one segment, its indices at idx + 256 c) */
static void gather_list(const cop_batch *b, const cop_tx_desc *t, const cop_tx_burst *o, const uint32_t *idx,
                        const uint32_t *count, int seg)
{
    const uint32_t n = b->n;
    const int imix = b->offsets != NULL;
    const uint32_t nchunk = n ? (n + COP_SEG_PKTS - 1) / COP_SEG_PKTS : 1;
    uint32_t k = 0, bytes = 0;   /* list position and byte base of the chunk */
    uint32_t W = 0, used = 0;
    int open = 1;                /* every earlier frame was written */
    const uint32_t dense = (!seg && n) ? (count[0] < n ? count[0] : n) : 0;
    for (uint32_t c = 0; c < nchunk; c++) {
        const uint32_t cap = n > c * COP_SEG_PKTS ? (n - c * COP_SEG_PKTS < COP_SEG_PKTS ? n - c * COP_SEG_PKTS : COP_SEG_PKTS) : 0;
        uint32_t cnt;
        if (!n) cnt = 0;
        else if (seg) cnt = count[c] < cap ? count[c] : cap;
        else cnt = dense > c * COP_SEG_PKTS ? (dense - c * COP_SEG_PKTS < COP_SEG_PKTS ? dense - c * COP_SEG_PKTS : COP_SEG_PKTS) : 0;
        for (uint32_t j = 0; j < cnt; j++, k++) {
            uint32_t i = idx[(size_t)c * COP_SEG_PKTS + j];
            if (i >= n) i = n - 1;
            uint32_t len, ext, off;
            if (imix) {
                len = t->lens[i];
                len = len < 1 ? 1 : len > COP_TX_MAX_FRAME ? COP_TX_MAX_FRAME : len;
                ext = (len + 15u) & ~15u;
                off = bytes;
            } else {
                len = ext = t->copy_bytes;
                off = k * t->slot_bytes;   /* used only where the frame fits (then < 2^32) */
            }
            bytes = imix ? bytes + ext : bytes;
            if (!open) continue;
            /* 64-bit: a slot frame's offset may pass 2^32 where it no longer fits */
            const uint64_t off64 = imix ? off : (uint64_t)k * t->slot_bytes;
            if (k >= o->cap_frames || off64 + ext > o->cap_bytes) {
                open = 0;
                continue;
            }
            const uint8_t *src = (const uint8_t *)b->pkts + (imix ? (uint64_t)b->offsets[i] : (uint64_t)i * b->stride) +
                                 b->data_off;
            memcpy((uint8_t *)o->frames + off, src, ext);
            if (o->off) o->off[k] = off;
            if (o->len) o->len[k] = len;
            W = k + 1;
            used = off + ext;
        }
    }
    o->status[0] = W;
    o->status[1] = used;
    o->status[2] = k - W;
    o->status[3] = 0;
}

int cop_tx_gather_host(const cop_batch *batches, const cop_tx_desc *tx, uint32_t nb, uint32_t n_lists, int seg,
                       uint32_t max_batch)
{
    if (nb == 0) return 0;
    if (cop_tx_validate(batches, tx, nb, n_lists, seg, max_batch, NULL)) return -EINVAL;
    for (uint32_t i = 0; i < nb; i++)
        for (uint32_t q = 0; q < n_lists; q++)
            gather_list(&batches[i], &tx[i], &tx[i].out[q],
                        batches[i].n ? batches[i].fwd_idx + (size_t)q * batches[i].n : NULL,
                        batches[i].n ? batches[i].fwd_count + q : NULL, seg);
    return 0;
}
