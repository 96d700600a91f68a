/*
 * lpm_live.c — rule-at-a-time changes to a host LPM table, and the patches
 * that carry them into a device DIR-24-8 image.
 *
 * cop_lpm_build (lpm_build.c) decides acceptance for a whole rule list and
 * flattens it with one sorted sweep. This file keeps the same table current
 * under rte_lpm_add / rte_lpm_delete / rte_lpm_delete_all without repeating
 * that sweep. Behind a table that is mutated sits an index, built at the
 * first mutation:
 *
 *   rmap     (depth, masked ip) -> rule id, with deletion
 *   pmap     /24 -> number of held rules deeper than 24 (DPDK's tbl8 group
 *            is in use while that number is not zero: tbl8_recycle_check)
 *   sorted   rule ids ordered by (ip, depth): the rules nested in a prefix
 *            are one contiguous run of it
 *   heap     freed rule ids, lowest first
 *
 * A mutation of prefix P = [st, en] changes the lookup function inside P
 * only. The new function on P is the sweep of lpm_build.c run over the rules
 * nested in P (a run of `sorted`), on top of the longest held rule that
 * covers P (at most 31 probes of rmap). The result replaces the entries of
 * the interval arrays that start inside [st, en + 1]; the seams are merged so
 * that the arrays stay canonical (neighbouring values differ), which makes
 * them equal to what a rebuild would give. n_ext, n_ext_rule and the report's
 * interval count are corrected from the entries removed and inserted. The
 * cost is the nested run plus two memmoves of the array tails.
 *
 * Every successful mutation bumps the generation and is appended to a ring
 * journal; cop_lpm_patch_records turns the journalled ranges since a device
 * image's generation into disjoint fill records for the patch kernel
 * (cop_patch.hip), allocating and releasing the image's tbl8 groups.
 */
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include "cop_internal.h"

static inline uint32_t depth_mask(uint32_t depth)
{
    return depth == 0 ? 0u : (uint32_t)(0xFFFFFFFFull << (32 - depth));
}

static inline uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

/* ---- open-addressing map u64 -> u32 with deletion (linear probing,
 * backward shift), kept at most half full --------------------------------- */
typedef struct {
    uint64_t *keys;
    uint32_t *vals;
    uint64_t  cap, n;
} lmap;
#define LMAP_EMPTY (~0ull)

static int lmap_alloc(lmap *m, uint64_t cap)
{
    m->keys = (uint64_t *)malloc(cap * sizeof(uint64_t));
    m->vals = (uint32_t *)malloc(cap * sizeof(uint32_t));
    if (!m->keys || !m->vals) {
        free(m->keys);
        free(m->vals);
        m->keys = NULL;
        m->vals = NULL;
        return -ENOMEM;
    }
    memset(m->keys, 0xFF, cap * sizeof(uint64_t));
    m->cap = cap;
    m->n = 0;
    return 0;
}

static void lmap_free(lmap *m)
{
    free(m->keys);
    free(m->vals);
    m->keys = NULL;
    m->vals = NULL;
}

static uint32_t *lmap_find(const lmap *m, uint64_t key)
{
    uint64_t i = mix64(key) & (m->cap - 1);
    for (;;) {
        if (m->keys[i] == key) return &m->vals[i];
        if (m->keys[i] == LMAP_EMPTY) return NULL;
        i = (i + 1) & (m->cap - 1);
    }
}

/* the key must be absent and room reserved */
static void lmap_put(lmap *m, uint64_t key, uint32_t val)
{
    uint64_t i = mix64(key) & (m->cap - 1);
    while (m->keys[i] != LMAP_EMPTY) i = (i + 1) & (m->cap - 1);
    m->keys[i] = key;
    m->vals[i] = val;
    m->n++;
}

static int lmap_reserve(lmap *m, uint64_t extra)
{
    if ((m->n + extra) * 2 <= m->cap) return 0;
    uint64_t cap = m->cap;
    while ((m->n + extra) * 2 > cap) cap <<= 1;
    lmap nm;
    if (lmap_alloc(&nm, cap)) return -ENOMEM;
    for (uint64_t i = 0; i < m->cap; i++)
        if (m->keys[i] != LMAP_EMPTY) lmap_put(&nm, m->keys[i], m->vals[i]);
    lmap_free(m);
    *m = nm;
    return 0;
}

static void lmap_erase(lmap *m, uint64_t key)
{
    const uint64_t mask = m->cap - 1;
    uint64_t i = mix64(key) & mask;
    for (;;) {
        if (m->keys[i] == key) break;
        if (m->keys[i] == LMAP_EMPTY) return;
        i = (i + 1) & mask;
    }
    m->n--;
    for (;;) {
        m->keys[i] = LMAP_EMPTY;
        uint64_t j = i;
        for (;;) {
            j = (j + 1) & mask;
            if (m->keys[j] == LMAP_EMPTY) return;
            const uint64_t k = mix64(m->keys[j]) & mask;   /* j's home slot */
            /* j may move into the hole i unless its home lies in (i, j] */
            if (i <= j ? (i < k && k <= j) : (i < k || k <= j)) continue;
            break;
        }
        m->keys[i] = m->keys[j];
        m->vals[i] = m->vals[j];
        i = j;
    }
}

static void lmap_clear(lmap *m)
{
    memset(m->keys, 0xFF, m->cap * sizeof(uint64_t));
    m->n = 0;
}

/* ---- the index behind a mutated table ---------------------------------- */
struct cop_lpm_live {
    lmap      rmap, pmap;
    uint32_t *sorted;
    uint32_t  n_sorted, cap_sorted;
    uint32_t *heap;
    uint32_t  n_heap, cap_heap;
    uint32_t  cap_rules, cap_iv;     /* entries allocated in rule_* and in iv_* / rv_* */
    cop_lpm_change *j;               /* ring: the change to generation g at j[g % j_cap] */
    uint32_t  j_cap, j_n;
};

uint64_t cop_lpm_next_uid(void)
{
    static uint64_t next;
    return __atomic_add_fetch(&next, 1, __ATOMIC_RELAXED);
}

void cop_lpm_live_free(struct cop_lpm_live *l)
{
    if (!l) return;
    lmap_free(&l->rmap);
    lmap_free(&l->pmap);
    free(l->sorted);
    free(l->heap);
    free(l->j);
    free(l);
}

static inline uint64_t rule_key(uint32_t ipm, uint32_t depth)
{
    return ((uint64_t)depth << 32) | ipm;
}

/* (ip, depth) order of the sorted index */
static inline int rule_before(const cop_lpm_table *t, uint32_t id, uint32_t ip, uint32_t depth)
{
    if (t->rule_ip[id] != ip) return t->rule_ip[id] < ip;
    return t->rule_depth[id] < depth;
}

/* first position of `sorted` whose rule is not before (ip, depth) */
static uint32_t sorted_lower(const cop_lpm_table *t, uint32_t ip, uint32_t depth)
{
    const struct cop_lpm_live *l = t->live;
    uint32_t lo = 0, hi = l->n_sorted;
    while (lo < hi) {
        uint32_t mid = lo + (hi - lo) / 2;
        if (rule_before(t, l->sorted[mid], ip, depth)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

typedef struct {
    uint32_t ip, id;
    uint8_t  depth;
} sortkey;

static int sortkey_cmp(const void *a, const void *b)
{
    const sortkey *x = (const sortkey *)a, *y = (const sortkey *)b;
    if (x->ip != y->ip) return x->ip < y->ip ? -1 : 1;
    return (int)x->depth - (int)y->depth;
}

static int grow_u32(uint32_t **p, uint32_t want)
{
    uint32_t *q = (uint32_t *)realloc(*p, (size_t)want * sizeof(uint32_t));
    if (!q) return -ENOMEM;
    *p = q;
    return 0;
}

/* room for one more rule: rule arrays, sorted index, id heap, both maps and
 * the interval arrays (at most 2 * rules + 1 intervals) */
static int live_reserve(cop_lpm_table *t)
{
    struct cop_lpm_live *l = t->live;
    if (t->n_rules + 1 > l->cap_rules) {
        uint32_t cap = l->cap_rules * 2;
        uint8_t *d = (uint8_t *)realloc(t->rule_depth, cap);
        if (d) t->rule_depth = d;
        if (!d || grow_u32(&t->rule_ip, cap) || grow_u32(&t->rule_nh, cap)) return -ENOMEM;
        l->cap_rules = cap;
    }
    if (l->n_sorted + 1 > l->cap_sorted) {
        if (grow_u32(&l->sorted, l->cap_sorted * 2)) return -ENOMEM;
        l->cap_sorted *= 2;
    }
    if (t->n_rules + 1 > l->cap_heap) {
        if (grow_u32(&l->heap, l->cap_heap * 2)) return -ENOMEM;
        l->cap_heap *= 2;
    }
    const uint32_t need = 2 * (t->n_held + 1) + 4;
    if (need > l->cap_iv) {
        uint32_t cap = l->cap_iv;
        while (cap < need) cap *= 2;
        if (grow_u32(&t->iv_start, cap) || grow_u32(&t->iv_val, cap) || grow_u32(&t->rv_start, cap) ||
            grow_u32(&t->rv_rule, cap))
            return -ENOMEM;
        l->cap_iv = cap;
    }
    if (lmap_reserve(&l->rmap, 1) || lmap_reserve(&l->pmap, 1)) return -ENOMEM;
    return 0;
}

/* build the index of a table that has none (first mutation) */
static int live_init(cop_lpm_table *t)
{
    if (t->live) return 0;
    struct cop_lpm_live *l = (struct cop_lpm_live *)calloc(1, sizeof(*l));
    if (!l) return -ENOMEM;
    const uint32_t n = t->n_rules;
    uint32_t cap = 16;
    while (cap < n + 1) cap *= 2;
    sortkey *sk = (sortkey *)malloc((size_t)(n ? n : 1) * sizeof(sortkey));
    l->sorted = (uint32_t *)malloc((size_t)cap * sizeof(uint32_t));
    l->heap = (uint32_t *)malloc((size_t)cap * sizeof(uint32_t));
    l->j = (cop_lpm_change *)malloc((size_t)COP_LPM_JOURNAL_CAP * sizeof(cop_lpm_change));
    uint64_t mcap = 32;
    while (mcap < ((uint64_t)n + 1) * 2) mcap <<= 1;
    int rc = (!sk || !l->sorted || !l->heap || !l->j) ? -ENOMEM : 0;
    if (!rc) rc = lmap_alloc(&l->rmap, mcap);
    if (!rc) rc = lmap_alloc(&l->pmap, 32);
    /* the arrays cop_lpm_build sized to its input grow to round capacities */
    if (!rc) {
        uint8_t *d = (uint8_t *)realloc(t->rule_depth, cap);
        if (d) t->rule_depth = d;
        if (!d || grow_u32(&t->rule_ip, cap) || grow_u32(&t->rule_nh, cap)) rc = -ENOMEM;
    }
    uint32_t icap = 16;
    while (icap < 2 * (n + 1) + 4) icap *= 2;
    if (!rc && (grow_u32(&t->iv_start, icap) || grow_u32(&t->iv_val, icap) || grow_u32(&t->rv_start, icap) ||
                grow_u32(&t->rv_rule, icap)))
        rc = -ENOMEM;
    if (rc) {
        free(sk);
        cop_lpm_live_free(l);
        return rc;
    }
    l->cap_sorted = l->cap_heap = l->cap_rules = cap;
    l->cap_iv = icap;
    l->j_cap = COP_LPM_JOURNAL_CAP;
    t->live = l;
    for (uint32_t i = 0; i < n; i++) {
        sk[i].ip = t->rule_ip[i];
        sk[i].depth = t->rule_depth[i];
        sk[i].id = i;
        lmap_put(&l->rmap, rule_key(t->rule_ip[i], t->rule_depth[i]), i);
        if (t->rule_depth[i] > 24) {
            if (lmap_reserve(&l->pmap, 1)) {
                rc = -ENOMEM;
                break;
            }
            uint32_t *cnt = lmap_find(&l->pmap, t->rule_ip[i] >> 8);
            if (cnt) (*cnt)++;
            else lmap_put(&l->pmap, t->rule_ip[i] >> 8, 1);
        }
    }
    if (rc) {
        free(sk);
        t->live = NULL;
        cop_lpm_live_free(l);
        return rc;
    }
    qsort(sk, n, sizeof(sortkey), sortkey_cmp);
    for (uint32_t i = 0; i < n; i++) l->sorted[i] = sk[i].id;
    l->n_sorted = n;
    free(sk);
    return 0;
}

int cop_lpm_index(cop_lpm_table *t)
{
    return t ? live_init(t) : -EINVAL;
}

/* ---- free rule ids, lowest first ---------------------------------------- */
static void heap_push(struct cop_lpm_live *l, uint32_t id)
{
    uint32_t i = l->n_heap++;
    while (i && l->heap[(i - 1) / 2] > id) {
        l->heap[i] = l->heap[(i - 1) / 2];
        i = (i - 1) / 2;
    }
    l->heap[i] = id;
}

static uint32_t heap_pop(struct cop_lpm_live *l)
{
    const uint32_t top = l->heap[0], last = l->heap[--l->n_heap];
    uint32_t i = 0;
    for (;;) {
        uint32_t c = 2 * i + 1;
        if (c >= l->n_heap) break;
        if (c + 1 < l->n_heap && l->heap[c + 1] < l->heap[c]) c++;
        if (l->heap[c] >= last) break;
        l->heap[i] = l->heap[c];
        i = c;
    }
    if (l->n_heap) l->heap[i] = last;
    return top;
}

/* ---- re-flattening one prefix's range ----------------------------------- */
typedef struct {
    uint32_t *start;
    uint32_t *val;
    uint32_t  n;
} ivbuf;

/* lpm_build.c's emit: keeps the list canonical (neighbouring values differ) */
static void iv_emit(ivbuf *b, uint64_t pos, uint32_t val)
{
    if (pos >= (1ull << 32)) return;
    if (b->n && b->start[b->n - 1] == (uint32_t)pos) {
        b->val[b->n - 1] = val;
        if (b->n >= 2 && b->val[b->n - 2] == val) b->n--;
        return;
    }
    if (b->n && b->val[b->n - 1] == val) return;
    b->start[b->n] = (uint32_t)pos;
    b->val[b->n] = val;
    b->n++;
}

/* first index with start[idx] > x (start[0] == 0, so the result is >= 1) */
static uint32_t iv_upper(const uint32_t *start, uint32_t n, uint32_t x)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        uint32_t mid = lo + (hi - lo) / 2;
        if (start[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

/* /24 blocks b_lo..b_hi with an interval start strictly inside */
static uint32_t ext_in_blocks(const uint32_t *start, uint32_t n, uint32_t b_lo, uint32_t b_hi)
{
    uint32_t k = b_lo ? iv_upper(start, n, (b_lo << 8) - 1) : 0;
    uint32_t cnt = 0, last = 0xFFFFFFFFu;
    for (; k < n && (start[k] >> 8) <= b_hi; k++) {
        if ((start[k] & 0xFFu) != 0 && (start[k] >> 8) != last) {
            cnt++;
            last = start[k] >> 8;
        }
    }
    return cnt;
}

/* entries of val[lo..hi] (clipped to n) that differ from their predecessor in
 * (nh | hit): their share of the merged interval count */
static uint32_t merged_in(const uint32_t *val, uint32_t n, uint32_t lo, uint32_t hi)
{
    uint32_t cnt = 0;
    for (uint32_t k = lo; k <= hi && k < n; k++)
        if (k == 0 || ((val[k] ^ val[k - 1]) & COP_IV_NHHIT)) cnt++;
    return cnt;
}

/* Replace the entries of (start, val, *n) that start in [st, en + 1] by the
 * canonical list (ns, nv, nn), whose first entry starts at st and whose last
 * restores the old value at en + 1. Returns through lo / len where the new
 * entries went. */
static void splice(uint32_t *start, uint32_t *val, uint32_t *n, uint32_t st, uint32_t en, const uint32_t *ns,
                   const uint32_t *nv, uint32_t nn, uint32_t *lo_out, uint32_t *hi_out, uint32_t *len_out)
{
    const uint32_t lo = st ? iv_upper(start, *n, st - 1) : 0;
    const uint32_t hi = en == 0xFFFFFFFFu ? *n : iv_upper(start, *n, en + 1);
    const uint32_t skip = (lo > 0 && nv[0] == val[lo - 1]) ? 1 : 0;   /* merges into the interval before st */
    const uint32_t len = nn - skip;
    memmove(start + lo + len, start + hi, (size_t)(*n - hi) * sizeof(uint32_t));
    memmove(val + lo + len, val + hi, (size_t)(*n - hi) * sizeof(uint32_t));
    memcpy(start + lo, ns + skip, (size_t)len * sizeof(uint32_t));
    memcpy(val + lo, nv + skip, (size_t)len * sizeof(uint32_t));
    *n = *n - (hi - lo) + len;
    *lo_out = lo;
    *hi_out = hi;
    *len_out = len;
}

/* Recompute the table's function on prefix [st, en] of depth d from the
 * rules now held. The caller has reserved the interval arrays. */
static int reflatten(cop_lpm_table *t, uint32_t st, uint32_t en, uint32_t d)
{
    struct cop_lpm_live *l = t->live;
    /* the longest held rule shallower than d that covers the range */
    uint32_t cval = 0, crule = COP_NO_RULE;
    for (uint32_t dd = d; dd-- > 1;) {
        const uint32_t *id = lmap_find(&l->rmap, rule_key(st & depth_mask(dd), dd));
        if (id) {
            crule = *id;
            cval = t->rule_nh[crule] | COP_IV_HIT | (dd << COP_IV_DEPTH_SH);
            break;
        }
    }
    /* the rules nested in the range: a run of the sorted index */
    const uint32_t s_lo = d ? sorted_lower(t, st, d) : 0;
    uint32_t s_hi = s_lo;
    while (s_hi < l->n_sorted && t->rule_ip[l->sorted[s_hi]] <= en) s_hi++;
    const uint32_t cap = 2 * (s_hi - s_lo) + 4;
    uint32_t *tmp = (uint32_t *)malloc((size_t)cap * 4 * sizeof(uint32_t));
    if (!tmp) return -ENOMEM;
    ivbuf b = {tmp, tmp + cap, 0}, br = {tmp + 2 * cap, tmp + 3 * cap, 0};
    /* the values just past the range do not change */
    uint32_t after_v = 0, after_r = COP_NO_RULE;
    if (en != 0xFFFFFFFFu) {
        after_v = t->iv_val[iv_upper(t->iv_start, t->n_iv, en + 1) - 1];
        after_r = t->rv_rule[iv_upper(t->rv_start, t->n_rv, en + 1) - 1];
    }
    iv_emit(&b, st, cval);
    iv_emit(&br, st, crule);
    struct {
        uint64_t end;
        uint32_t val, rule;
    } stk[COP_LPM_MAX_DEPTH + 2];
    int sp = 0;
    for (uint32_t i = s_lo; i < s_hi; i++) {
        const uint32_t id = l->sorted[i];
        const uint64_t rs = t->rule_ip[id], re = rs + (1ull << (32 - t->rule_depth[id])) - 1;
        while (sp > 0 && stk[sp - 1].end < rs) {
            sp--;
            if (stk[sp].end < en) {
                iv_emit(&b, stk[sp].end + 1, sp ? stk[sp - 1].val : cval);
                iv_emit(&br, stk[sp].end + 1, sp ? stk[sp - 1].rule : crule);
            }
        }
        const uint32_t v = t->rule_nh[id] | COP_IV_HIT | ((uint32_t)t->rule_depth[id] << COP_IV_DEPTH_SH);
        iv_emit(&b, rs, v);
        iv_emit(&br, rs, id);
        stk[sp].end = re;
        stk[sp].val = v;
        stk[sp].rule = id;
        sp++;
    }
    while (sp > 0) {
        sp--;
        if (stk[sp].end < en) {
            iv_emit(&b, stk[sp].end + 1, sp ? stk[sp - 1].val : cval);
            iv_emit(&br, stk[sp].end + 1, sp ? stk[sp - 1].rule : crule);
        }
    }
    if (en != 0xFFFFFFFFu) {
        iv_emit(&b, (uint64_t)en + 1, after_v);
        iv_emit(&br, (uint64_t)en + 1, after_r);
    }

    const uint32_t b_lo = st >> 8, b_hi = (en == 0xFFFFFFFFu ? en : en + 1) >> 8;
    uint32_t lo, hi, len;
    uint32_t ext0 = ext_in_blocks(t->iv_start, t->n_iv, b_lo, b_hi);
    /* the merged count's share: the replaced entries and the one after them */
    const uint32_t m_lo = st ? iv_upper(t->iv_start, t->n_iv, st - 1) : 0;
    const uint32_t m_hi = en == 0xFFFFFFFFu ? t->n_iv : iv_upper(t->iv_start, t->n_iv, en + 1);
    const uint32_t mg0 = merged_in(t->iv_val, t->n_iv, m_lo, m_hi);
    splice(t->iv_start, t->iv_val, &t->n_iv, st, en, b.start, b.val, b.n, &lo, &hi, &len);
    t->n_ext = t->n_ext - ext0 + ext_in_blocks(t->iv_start, t->n_iv, b_lo, b_hi);
    t->report.n_intervals = t->report.n_intervals - mg0 + merged_in(t->iv_val, t->n_iv, lo, lo + len);

    ext0 = ext_in_blocks(t->rv_start, t->n_rv, b_lo, b_hi);
    splice(t->rv_start, t->rv_rule, &t->n_rv, st, en, br.start, br.val, br.n, &lo, &hi, &len);
    t->n_ext_rule = t->n_ext_rule - ext0 + ext_in_blocks(t->rv_start, t->n_rv, b_lo, b_hi);
    free(tmp);
    return 0;
}

static void journal_push(cop_lpm_table *t, uint32_t ip, uint32_t depth, uint32_t id, int kind)
{
    struct cop_lpm_live *l = t->live;
    t->generation++;
    cop_lpm_change *c = &l->j[t->generation % l->j_cap];
    c->ip = ip;
    c->id = id;
    c->depth = (uint8_t)depth;
    c->kind = (uint8_t)kind;
    if (l->j_n < l->j_cap) l->j_n++;
    t->report.n_distinct = t->n_held;
    t->report.tbl8_used = t->tbl8_used;
}

/* ---- the public calls --------------------------------------------------- */
int cop_lpm_create(const cop_lpm_config *cfg, cop_lpm_table **out)
{
    cop_lpm_config dflt = {COP_FW_MAX_RULES, COP_FW_NUMBER_TBL8S, COP_LPM_STOP_AT_FIRST_ERROR};
    return cop_lpm_build(NULL, 0, cfg ? cfg : &dflt, out, NULL);
}

int cop_lpm_add(cop_lpm_table *t, uint32_t ip, uint8_t depth, uint32_t next_hop)
{
    if (!t || depth < 1 || depth > COP_LPM_MAX_DEPTH) return -EINVAL;
    int rc = live_init(t);
    if (rc) return rc;
    struct cop_lpm_live *l = t->live;
    const uint32_t ipm = ip & depth_mask(depth), en = ipm | ~depth_mask(depth);
    next_hop &= COP_LPM_NH_MASK;
    uint32_t *held = lmap_find(&l->rmap, rule_key(ipm, depth));
    if (held) {
        const uint32_t id = *held, old = t->rule_nh[id];
        t->rule_nh[id] = next_hop;
        if ((rc = reflatten(t, ipm, en, depth)) != 0) {
            t->rule_nh[id] = old;
            return rc;
        }
        journal_push(t, ipm, depth, id, COP_CHG_SET);
        return 0;
    }
    if (t->n_held >= t->cfg.max_rules) return -ENOSPC;
    uint32_t *deep = depth > 24 ? lmap_find(&l->pmap, ipm >> 8) : NULL;
    if (depth > 24 && !deep && t->tbl8_used >= t->cfg.number_tbl8s) return -ENOSPC;
    if ((rc = live_reserve(t)) != 0) return rc;
    if (depth > 24) {
        deep = lmap_find(&l->pmap, ipm >> 8);   /* (the reserve may have moved the map) */
        if (deep) {
            (*deep)++;
        } else {
            lmap_put(&l->pmap, ipm >> 8, 1);
            t->tbl8_used++;
        }
    }
    const uint32_t id = l->n_heap ? heap_pop(l) : t->n_rules++;
    t->rule_ip[id] = ipm;
    t->rule_depth[id] = depth;
    t->rule_nh[id] = next_hop;
    t->n_held++;
    lmap_put(&l->rmap, rule_key(ipm, depth), id);
    const uint32_t pos = sorted_lower(t, ipm, depth);
    memmove(l->sorted + pos + 1, l->sorted + pos, (size_t)(l->n_sorted - pos) * sizeof(uint32_t));
    l->sorted[pos] = id;
    l->n_sorted++;
    if ((rc = reflatten(t, ipm, en, depth)) != 0) {
        /* out of memory for the sweep's scratch: take the rule out again */
        memmove(l->sorted + pos, l->sorted + pos + 1, (size_t)(l->n_sorted - pos - 1) * sizeof(uint32_t));
        l->n_sorted--;
        lmap_erase(&l->rmap, rule_key(ipm, depth));
        t->rule_depth[id] = 0;
        t->n_held--;
        if (id == t->n_rules - 1) t->n_rules--;
        else heap_push(l, id);
        if (depth > 24) {
            deep = lmap_find(&l->pmap, ipm >> 8);
            if (--(*deep) == 0) {
                lmap_erase(&l->pmap, ipm >> 8);
                t->tbl8_used--;
            }
        }
        return rc;
    }
    journal_push(t, ipm, depth, id, COP_CHG_ADD);
    return 0;
}

int cop_lpm_delete(cop_lpm_table *t, uint32_t ip, uint8_t depth)
{
    if (!t || depth < 1 || depth > COP_LPM_MAX_DEPTH) return -EINVAL;
    int rc = live_init(t);
    if (rc) return rc;
    struct cop_lpm_live *l = t->live;
    const uint32_t ipm = ip & depth_mask(depth), en = ipm | ~depth_mask(depth);
    const uint32_t *held = lmap_find(&l->rmap, rule_key(ipm, depth));
    if (!held) return -EINVAL;   /* rte_lpm_delete: rule_find < 0 -> -EINVAL */
    const uint32_t id = *held;
    const uint32_t pos = sorted_lower(t, ipm, depth);
    memmove(l->sorted + pos, l->sorted + pos + 1, (size_t)(l->n_sorted - pos - 1) * sizeof(uint32_t));
    l->n_sorted--;
    lmap_erase(&l->rmap, rule_key(ipm, depth));
    if ((rc = reflatten(t, ipm, en, depth)) != 0) {
        memmove(l->sorted + pos + 1, l->sorted + pos, (size_t)(l->n_sorted - pos) * sizeof(uint32_t));
        l->sorted[pos] = id;
        l->n_sorted++;
        lmap_put(&l->rmap, rule_key(ipm, depth), id);
        return rc;
    }
    if (depth > 24) {
        uint32_t *deep = lmap_find(&l->pmap, ipm >> 8);
        if (--(*deep) == 0) {   /* tbl8_recycle_check: the group's last deep rule left */
            lmap_erase(&l->pmap, ipm >> 8);
            t->tbl8_used--;
        }
    }
    t->rule_depth[id] = 0;
    t->rule_nh[id] = 0;
    t->n_held--;
    heap_push(l, id);   /* (the heap holds n_rules ids: live_reserve sized it) */
    journal_push(t, ipm, depth, id, COP_CHG_DEL);
    return 0;
}

int cop_lpm_delete_all(cop_lpm_table *t)
{
    if (!t) return -EINVAL;
    int rc = live_init(t);
    if (rc) return rc;
    struct cop_lpm_live *l = t->live;
    lmap_clear(&l->rmap);
    lmap_clear(&l->pmap);
    l->n_sorted = l->n_heap = 0;
    memset(t->rule_depth, 0, l->cap_rules);
    t->n_rules = t->n_held = t->tbl8_used = 0;
    t->n_iv = t->n_rv = 1;
    t->iv_start[0] = t->rv_start[0] = 0;
    t->iv_val[0] = 0;
    t->rv_rule[0] = COP_NO_RULE;
    t->n_ext = t->n_ext_rule = 0;
    t->report.n_intervals = 1;
    journal_push(t, 0, 0, 0, COP_CHG_DEL_ALL);
    return 0;
}

int cop_lpm_is_rule_present(const cop_lpm_table *t, uint32_t ip, uint8_t depth, uint32_t *next_hop)
{
    if (!t || depth < 1 || depth > COP_LPM_MAX_DEPTH) return -EINVAL;
    const uint32_t ipm = ip & depth_mask(depth);
    uint32_t id = COP_NO_RULE;
    if (t->live) {
        const uint32_t *held = lmap_find(&t->live->rmap, rule_key(ipm, depth));
        if (held) id = *held;
    } else {
        /* never mutated: no index yet, and a const call builds none */
        for (uint32_t i = 0; i < t->n_rules && id == COP_NO_RULE; i++)
            if (t->rule_depth[i] == depth && t->rule_ip[i] == ipm) id = i;
    }
    if (id == COP_NO_RULE) return 0;
    if (next_hop) *next_hop = t->rule_nh[id];
    return 1;
}

void cop_lpm_report_get(const cop_lpm_table *t, cop_lpm_report *out)
{
    if (t && out) *out = t->report;
}

uint64_t cop_lpm_generation(const cop_lpm_table *t)
{
    return t ? t->generation : 0;
}

int cop_lpm_export_rules_ids(const cop_lpm_table *t, cop_prefix *out, uint32_t *ids, uint32_t cap)
{
    if (!t) return -EINVAL;
    if (!out || !ids) return (int)t->n_held;
    if (t->n_held > cap) return -ENOSPC;
    uint32_t k = 0;
    for (uint32_t i = 0; i < t->n_rules; i++) {
        if (!t->rule_depth[i]) continue;
        memset(&out[k], 0, sizeof(out[k]));
        out[k].ip = t->rule_ip[i];
        out[k].depth = t->rule_depth[i];
        out[k].next_hop = t->rule_nh[i];
        ids[k++] = i;
    }
    return (int)k;
}

/* ---- the journal --------------------------------------------------------- */
int cop_lpm_changes_since(const cop_lpm_table *t, uint64_t since, cop_lpm_change **out)
{
    if (!t || !out || since > t->generation) return -EINVAL;
    *out = NULL;
    const uint64_t cnt = t->generation - since;
    if (!cnt) return 0;
    const struct cop_lpm_live *l = t->live;
    if (cnt > l->j_n) return -ESTALE;
    cop_lpm_change *c = (cop_lpm_change *)malloc((size_t)cnt * sizeof(*c));
    if (!c) return -ENOMEM;
    for (uint64_t g = since + 1; g <= t->generation; g++) c[g - since - 1] = l->j[g % l->j_cap];
    *out = c;
    return (int)cnt;
}

int cop_lpm_journal_set_cap(cop_lpm_table *t, uint32_t cap)
{
    if (!t || !cap) return -EINVAL;
    int rc = live_init(t);
    if (rc) return rc;
    struct cop_lpm_live *l = t->live;
    cop_lpm_change *nj = (cop_lpm_change *)malloc((size_t)cap * sizeof(*nj));
    if (!nj) return -ENOMEM;
    const uint32_t keep = l->j_n < cap ? l->j_n : cap;
    for (uint64_t g = t->generation - keep + 1; g <= t->generation; g++) nj[g % cap] = l->j[g % l->j_cap];
    free(l->j);
    l->j = nj;
    l->j_cap = cap;
    l->j_n = keep;
    return 0;
}

/* ---- patches for a device DIR-24-8 image --------------------------------- */
struct cop_live_img {
    int       form;
    uint64_t  gen, uid;
    lmap      grp;          /* /24 block -> tbl8 group */
    uint32_t *freeg;        /* released groups (stack) */
    uint32_t  n_free;
    uint32_t  cap_groups, hw;   /* groups 0..hw-1 have been handed out */
};

void cop_live_img_free(cop_live_img *img)
{
    if (!img) return;
    lmap_free(&img->grp);
    free(img->freeg);
    free(img);
}

uint64_t cop_live_img_generation(const cop_live_img *img) { return img->gen; }
uint32_t cop_live_img_groups_used(const cop_live_img *img) { return (uint32_t)img->grp.n; }

cop_live_img *cop_live_img_create(const cop_lpm_table *t, int form, uint32_t cap_groups)
{
    const uint32_t *start = form == COP_FORM_RULE ? t->rv_start : t->iv_start;
    const uint32_t n = form == COP_FORM_RULE ? t->n_rv : t->n_iv;
    const uint32_t n_ext = cop_lpm_form_n_ext(t, form);
    if (cap_groups < n_ext) return NULL;
    cop_live_img *img = (cop_live_img *)calloc(1, sizeof(*img));
    if (!img) return NULL;
    uint64_t mcap = 32;
    while (mcap < ((uint64_t)n_ext + 1) * 2) mcap <<= 1;
    img->freeg = (uint32_t *)malloc((size_t)(cap_groups ? cap_groups : 1) * sizeof(uint32_t));
    if (!img->freeg || lmap_alloc(&img->grp, mcap)) {
        free(img->freeg);
        free(img);
        return NULL;
    }
    /* cop_lpm_form_fill_dir24's numbering: extended blocks in address order */
    uint32_t last = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < n; k++) {
        if ((start[k] & 0xFFu) != 0 && (start[k] >> 8) != last) {
            last = start[k] >> 8;
            lmap_put(&img->grp, last, img->hw++);
        }
    }
    img->form = form;
    img->gen = t->generation;
    img->uid = t->uid;
    img->cap_groups = cap_groups;
    return img;
}

typedef struct {
    cop_patch_rec *r;
    uint32_t n, cap;
    int oom;
} recvec;

static void rec_push(recvec *v, uint32_t table, uint32_t first, uint32_t count, uint32_t entry)
{
    if (v->n == v->cap) {
        uint32_t cap = v->cap ? v->cap * 2 : 64;
        cop_patch_rec *q = (cop_patch_rec *)realloc(v->r, (size_t)cap * sizeof(*q));
        if (!q) {
            v->oom = 1;
            return;
        }
        v->r = q;
        v->cap = cap;
    }
    cop_patch_rec *p = &v->r[v->n++];
    p->table = table;
    p->first = first;
    p->count = count;
    p->entry = entry;
}

typedef struct {
    const cop_lpm_table *t;
    const uint32_t *start, *val;
    uint32_t n;
    int form;
} formview;

static inline uint32_t fv_entry(const formview *f, uint32_t k)
{
    return f->form == COP_FORM_RULE ? cop_rule_entry(f->t, f->val[k]) : cop_dir_entry(f->val[k]);
}

static inline uint64_t fv_next(const formview *f, uint32_t k)
{
    return k + 1 < f->n ? f->start[k + 1] : (1ull << 32);
}

/* addresses a0..a1 of one /24 into group g, one record per interval */
static void paint_group(recvec *v, const formview *f, uint32_t g, uint32_t a0, uint32_t a1, cop_update_report *rep)
{
    uint32_t k = iv_upper(f->start, f->n, a0) - 1, a = a0;
    for (;;) {
        const uint64_t next = fv_next(f, k);
        const uint32_t run_end = next - 1 < a1 ? (uint32_t)(next - 1) : a1;
        rec_push(v, 1, g * 256 + (a & 0xFFu), run_end - a + 1, fv_entry(f, k));
        rep->tbl8_entries += run_end - a + 1;
        if (run_end == a1) return;
        a = run_end + 1;
        k++;
    }
}

static int take_group(cop_live_img *img, uint32_t *g)
{
    if (img->n_free) *g = img->freeg[--img->n_free];
    else if (img->hw < img->cap_groups) *g = img->hw++;
    else return -ENOSPC;
    return 0;
}

static int u32_cmp(const void *a, const void *b)
{
    const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
    return x < y ? -1 : x > y;
}

/* one maximal changed range [st, en] (a prefix: aligned, a power of two long).
 * *whole: the last /24 block this update has already written as a whole (its
 * tbl24 entry, or all 256 entries of a group it took): ranges come in address
 * order, and a later range inside that block has nothing left to write. */
static int patch_range(const formview *f, cop_live_img *img, recvec *v, uint32_t st, uint32_t en,
                       cop_update_report *rep, uint32_t *whole)
{
    const uint32_t b0 = st >> 8, b1 = en >> 8;
    if (en - st < 255) {
        /* deeper than /24: part of one block */
        if (*whole == b0) return 0;
        const uint32_t lo = b0 << 8, k0 = iv_upper(f->start, f->n, lo) - 1;
        const int interior = fv_next(f, k0) <= (uint64_t)lo + 255;
        uint32_t *has = lmap_find(&img->grp, b0);
        if (interior && has) {
            paint_group(v, f, *has, st, en, rep);
        } else if (interior) {
            uint32_t g;
            if (take_group(img, &g) || lmap_reserve(&img->grp, 1)) return -ENOSPC;
            lmap_put(&img->grp, b0, g);
            paint_group(v, f, g, lo, lo + 255, rep);
            rec_push(v, 0, b0, 1, g | COP_DIR_VALID_EXT);
            rep->tbl24_entries++;
            rep->groups_taken++;
            *whole = b0;
        } else {
            *whole = b0;
            if (has) {
                img->freeg[img->n_free++] = *has;
                lmap_erase(&img->grp, b0);
                rep->groups_released++;
            }
            rec_push(v, 0, b0, 1, fv_entry(f, k0));
            rep->tbl24_entries++;
        }
        return 0;
    }
    /* whole blocks b0..b1. The groups the image holds in them, ascending:
     * probe every block, or scan the book, whichever is less work */
    uint32_t *old = NULL, n_old = 0;
    if (img->grp.n) {
        old = (uint32_t *)malloc((size_t)img->grp.n * sizeof(uint32_t));
        if (!old) return -ENOMEM;
        if ((uint64_t)b1 - b0 + 1 <= img->grp.cap) {
            for (uint32_t b = b0;; b++) {
                if (lmap_find(&img->grp, b)) old[n_old++] = b;
                if (b == b1) break;
            }
        } else {
            for (uint64_t i = 0; i < img->grp.cap; i++)
                if (img->grp.keys[i] != LMAP_EMPTY && img->grp.keys[i] >= b0 && img->grp.keys[i] <= b1)
                    old[n_old++] = (uint32_t)img->grp.keys[i];
            qsort(old, n_old, sizeof(uint32_t), u32_cmp);
        }
    }
    int rc = 0;
    uint32_t oi = 0, b = b0, k = iv_upper(f->start, f->n, b0 << 8) - 1;
    for (;;) {
        const uint32_t lo = b << 8;
        while (fv_next(f, k) <= lo) k++;
        const uint64_t next = fv_next(f, k);
        uint32_t eb;   /* last block this step covers */
        if (next > (uint64_t)lo + 255) {
            /* plain blocks: all those that end before the next boundary */
            eb = (uint32_t)(next >> 8) - 1;
            if (eb > b1) eb = b1;
            rec_push(v, 0, b, eb - b + 1, fv_entry(f, k));
            rep->tbl24_entries += eb - b + 1;
            for (; oi < n_old && old[oi] <= eb; oi++) {   /* their groups go back */
                img->freeg[img->n_free++] = *lmap_find(&img->grp, old[oi]);
                lmap_erase(&img->grp, old[oi]);
                rep->groups_released++;
            }
        } else {
            eb = b;
            uint32_t g;
            if (oi < n_old && old[oi] == b) {
                g = *lmap_find(&img->grp, b);   /* keeps its group: tbl24 already points at it */
                oi++;
            } else {
                if (take_group(img, &g) || lmap_reserve(&img->grp, 1)) {
                    rc = -ENOSPC;
                    break;
                }
                lmap_put(&img->grp, b, g);
                rec_push(v, 0, b, 1, g | COP_DIR_VALID_EXT);
                rep->tbl24_entries++;
                rep->groups_taken++;
            }
            paint_group(v, f, g, lo, lo + 255, rep);
        }
        if (eb == b1) break;
        b = eb + 1;
    }
    free(old);
    return rc;
}

typedef struct {
    uint32_t st, en;
} range;

static int range_cmp(const void *a, const void *b)
{
    const range *x = (const range *)a, *y = (const range *)b;
    if (x->st != y->st) return x->st < y->st ? -1 : 1;
    return x->en > y->en ? -1 : x->en < y->en;   /* the wider first */
}

int cop_lpm_patch_records(const cop_lpm_table *t, cop_live_img *img, cop_patch_rec **recs, uint32_t *n,
                          cop_update_report *rep)
{
    if (!t || !img || !recs || !n || img->uid != t->uid) return -EINVAL;
    cop_update_report r;
    memset(&r, 0, sizeof(r));
    *recs = NULL;
    *n = 0;
    cop_lpm_change *chg = NULL;
    const int nc = cop_lpm_changes_since(t, img->gen, &chg);
    if (nc < 0) return nc;
    r.n_changes = (uint32_t)nc;
    /* the changed prefixes nest or are disjoint: keep the outermost ones */
    range *rg = (range *)malloc((size_t)(nc ? nc : 1) * sizeof(range));
    if (!rg) {
        free(chg);
        return -ENOMEM;
    }
    for (int i = 0; i < nc; i++) {
        rg[i].st = chg[i].ip;
        rg[i].en = chg[i].ip | ~depth_mask(chg[i].depth);
    }
    free(chg);
    qsort(rg, (size_t)nc, sizeof(range), range_cmp);
    formview f = {t, img->form == COP_FORM_RULE ? t->rv_start : t->iv_start,
                  img->form == COP_FORM_RULE ? t->rv_rule : t->iv_val, img->form == COP_FORM_RULE ? t->n_rv : t->n_iv,
                  img->form};
    recvec v = {NULL, 0, 0, 0};
    int rc = 0;
    uint64_t done = 0;   /* addresses below it are covered */
    uint32_t whole = 0xFFFFFFFFu;
    for (int i = 0; i < nc && !rc; i++) {
        if (rg[i].st < done) continue;   /* nested in the range before */
        rc = patch_range(&f, img, &v, rg[i].st, rg[i].en, &r, &whole);
        done = (uint64_t)rg[i].en + 1;
    }
    free(rg);
    if (!rc && v.oom) rc = -ENOMEM;
    if (rc) {
        free(v.r);
        return rc;
    }
    img->gen = t->generation;
    r.n_records = v.n;
    if (rep) *rep = r;
    *recs = v.r;
    *n = v.n;
    return 0;
}

int cop_patch_apply_host(uint32_t *tbl24, uint32_t cap24, uint32_t *tbl8, uint32_t cap8, const cop_patch_rec *recs,
                         uint32_t n)
{
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t cap = recs[i].table ? cap8 : cap24;
        if (recs[i].table > 1 || recs[i].first > cap || recs[i].count > cap - recs[i].first) return -EINVAL;
    }
    for (uint32_t i = 0; i < n; i++) {
        uint32_t *p = (recs[i].table ? tbl8 : tbl24) + recs[i].first;
        for (uint32_t k = 0; k < recs[i].count; k++) p[k] = recs[i].entry;
    }
    return 0;
}
