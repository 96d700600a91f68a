/*
 * lpm_lookup.c — host reference of the bulk lookups (cop_lookup_bulk) and
 * the probe set of cop_lookup_audit.
 *
 * The device answers a bulk lookup from whichever image the stage holds (LDS
 * intervals, DIR-24-8 with plain or packed tbl8 groups, trie, bucketed
 * intervals); all of them encode the merged (start, entry) intervals of
 * cop_lpm_form_intervals, which follows every live mutation of the table. The
 * reference is therefore a binary search over those intervals plus the mask
 * that strips what an image carries beyond the public word: the depth in
 * bits 26..31 of a next-hop entry and valid_group (bit 25) of a tbl8 entry.
 */
#include <errno.h>
#include <stdlib.h>

#include "cop_internal.h"

/* the public word of a device entry: e & mask when the hit bit is set, else 0 */
static inline uint32_t lookup_word(uint32_t e, uint32_t mask)
{
    return (e & COP_LOOKUP_HIT) ? (e & mask) : 0u;
}

int cop_lpm_lookup_words(const cop_lpm_table *t, int form, const uint32_t *ips, uint32_t n, uint32_t *out)
{
    if (!t || (form != COP_LOOKUP_NH && form != COP_LOOKUP_RULE) || (n && (!ips || !out))) return -EINVAL;
    if (n == 0) return 0;
    uint32_t *s = NULL, *v = NULL;
    const uint32_t m = cop_lpm_form_intervals(t, form, &s, &v);
    if (!s) return -ENOMEM;
    const uint32_t mask = form == COP_LOOKUP_RULE ? COP_LOOKUP_RULE_MASK : COP_LOOKUP_NH_MASK;
    for (uint32_t i = 0; i < n; i++) {
        /* last interval with start <= ip (starts[0] == 0) */
        uint32_t lo = 0, hi = m;
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (s[mid] <= ips[i]) lo = mid;
            else hi = mid;
        }
        out[i] = m ? lookup_word(v[lo], mask) : 0u;
    }
    free(s);
    free(v);
    return 0;
}

int cop_lpm_audit_probes(const cop_lpm_table *t, int form, uint32_t **ips, uint32_t *n)
{
    if (!t || (form != COP_LOOKUP_NH && form != COP_LOOKUP_RULE) || !ips || !n) return -EINVAL;
    *ips = NULL;
    *n = 0;
    uint32_t *s = NULL, *v = NULL;
    const uint32_t m = cop_lpm_form_intervals(t, form, &s, &v);
    if (!s) return -ENOMEM;
    free(v);
    uint32_t *p = (uint32_t *)malloc(((size_t)2 * m + 1) * sizeof(uint32_t));
    if (!p) {
        free(s);
        return -ENOMEM;
    }
    /* starts ascend, so s - 1 >= the start before it: the list ascends as it
     * is written, and an address equal to the last one written is a repeat */
    uint32_t k = 0;
    for (uint32_t i = 0; i < m; i++) {
        if (s[i] > 0 && (k == 0 || p[k - 1] != s[i] - 1u)) p[k++] = s[i] - 1u;
        if (k == 0 || p[k - 1] != s[i]) p[k++] = s[i];
    }
    if (k == 0 || p[k - 1] != 0xFFFFFFFFu) p[k++] = 0xFFFFFFFFu;
    free(s);
    *ips = p;
    *n = k;
    return 0;
}
