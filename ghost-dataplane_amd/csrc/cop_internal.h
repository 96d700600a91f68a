/*
 * cop_internal.h — host-side structures shared between the C setup code
 * (LPM builder, rules loader) and the HIP runtime. Not part of the ABI.
 */
#ifndef COP_INTERNAL_H
#define COP_INTERNAL_H

#include <stdint.h>
#include "cop_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Internal interval value: bits 0-23 next hop, bit 24 hit, bits 26-31 depth
 * of the matching rule (0 on a miss). Lookups only observe bits 0-24. */
#define COP_IV_HIT      0x01000000u
#define COP_IV_NHHIT    0x01FFFFFFu
#define COP_IV_DEPTH_SH 26

/* DIR-24-8 entry bits (DPDK v1604 rte_lpm_tbl_entry, little-endian). */
#define COP_DIR_VALID     0x01000000u
#define COP_DIR_EXT       0x02000000u
#define COP_DIR_VALID_EXT 0x03000000u

struct cop_lpm_table {
    /* accepted rule set (masked prefix, depth, final next hop) */
    uint32_t  n_rules;
    uint32_t *rule_ip;
    uint8_t  *rule_depth;
    uint32_t *rule_nh;
    /* flattened function over [0, 2^32): starts ascending, starts[0] = 0 */
    uint32_t  n_iv;
    uint32_t *iv_start;
    uint32_t *iv_val;      /* internal value incl. depth */
    uint32_t  tbl8_used;   /* DPDK-semantics tbl8 groups (acceptance) */
    uint32_t  n_ext;       /* /24 blocks that need a tbl8 group in our image */
    /* the same function keyed by matching rule id (index into rule_*;
     * COP_NO_RULE on a miss): the firewall's device image form */
    uint32_t  n_rv;
    uint32_t *rv_start;
    uint32_t *rv_rule;
    uint32_t  n_ext_rule;
    cop_lpm_report report;
    /* live tables (lpm_live.c): n_rules is the id space (highest id held so
     * far + 1), rule_depth[id] == 0 marks an id freed by cop_lpm_delete and
     * n_held counts the rules held. A table never deleted from has
     * n_held == n_rules. The index behind add / delete is built at the first
     * mutation, so a table that is only built and uploaded pays nothing. */
    cop_lpm_config cfg;
    uint32_t  n_held;
    uint64_t  generation;        /* successful mutations since the build */
    uint64_t  uid;               /* identity of this table object (never reused) */
    struct cop_lpm_live *live;
};

#define COP_NO_RULE 0xFFFFFFFFu

/* Device image forms. NH: entry = next_hop | VALID (the route stage).
 * RULE: entry = rule_id | VALID | DROP (bit 26: the rule's next hop, i.e.
 * its firewall action, is non-zero) — the firewall stage, which needs the
 * verdict and the matching rule (per-rule hit counters), not the action. */
enum { COP_FORM_NH = 0, COP_FORM_RULE = 1 };
#define COP_RV_DROP 0x04000000u

/* Merged (start, device entry) intervals of a form; arrays are malloc-ed. */
uint32_t cop_lpm_form_intervals(const cop_lpm_table *t, int form, uint32_t **starts, uint32_t **entries);
/* /24 blocks with an interior boundary in a form's image (tbl8 groups). */
uint32_t cop_lpm_form_n_ext(const cop_lpm_table *t, int form);
/* Paint a form's DIR-24-8 image (tbl24: 1<<24, tbl8: n_ext(form) * 256). */
void cop_lpm_form_fill_dir24(const cop_lpm_table *t, int form, uint32_t *tbl24, uint32_t *tbl8);

/* Flatten (hit,nh) only: merged interval arrays for the LDS search form.
 * Returns the count; the starts and vals arrays are malloc-ed. */
uint32_t cop_lpm_merged_intervals(const cop_lpm_table *t, uint32_t **starts, uint32_t **vals);
/* Build the DIR-24-8 image into caller buffers (tbl24: 1<<24 entries,
 * tbl8: t->n_ext * 256 entries). */
void cop_lpm_fill_dir24(const cop_lpm_table *t, uint32_t *tbl24, uint32_t *tbl8);

/* Multibit-trie device form (lpm_trie.c): a 12-bit top level (LDS), then
 * popcount-compressed 6-bit nodes of COP_TRIE_NODE_WORDS u32 and a leaf
 * array (L2-resident). Level-0 entries with COP_TRIE_NODE set are nodes. */
#define COP_TRIE_L0 4096u
#define COP_TRIE_NODE 0x80000000u
#define COP_TRIE_NODE_WORDS 6u
typedef struct {
    uint32_t l0[COP_TRIE_L0];
    uint32_t n_nodes, n_leaves;
    uint32_t *nodes;    /* n_nodes * COP_TRIE_NODE_WORDS */
    uint32_t *leaves;
} cop_lpm_trie;
int cop_lpm_trie_build(const uint32_t *starts, const uint32_t *vals, uint32_t m, cop_lpm_trie *out);
void cop_lpm_trie_free(cop_lpm_trie *t);
uint32_t cop_lpm_trie_lookup(const cop_lpm_trie *t, uint32_t ip);
/* tests: the trie of a table's form; per ip the trie walk (out) and the
 * interval search (ref); node and leaf counts */
int cop_lpm_trie_probe(const cop_lpm_table *tab, int form, const uint32_t *ips, uint32_t n, uint32_t *out,
                       uint32_t *ref, uint32_t *n_nodes, uint32_t *n_leaves);

/* Bucketed interval device form (lpm_bkt.c, COP_CFG_LPM_BKT): idx = 2^ib + 1
 * first-candidate positions, pairs = (start, value) x (m + COP_BKT_PADS) */
#define COP_BKT_MIN_BITS 12u
#define COP_BKT_MAX_BITS 22u
#define COP_BKT_PADS 8u
#define COP_BKT_XBITS 1u   /* default: 2 buckets per interval */
typedef struct {
    uint32_t m, ib, lv, widest;
    uint32_t *idx;
    uint32_t *pairs;
} cop_lpm_bkt;
int cop_lpm_bkt_build(const uint32_t *starts, const uint32_t *vals, uint32_t m, uint32_t xbits, cop_lpm_bkt *out);
void cop_lpm_bkt_free(cop_lpm_bkt *t);
uint32_t cop_lpm_bkt_lookup(const cop_lpm_bkt *t, uint32_t ip, uint32_t *rounds);
/* tests: the bucketed form of a table's form; per ip its lookup (out) and
 * the binary search over all intervals (ref); info = {m, ib, lv, widest,
 * lookups that needed a wide-bucket round, the wide-bucket rounds} */
int cop_lpm_bkt_probe(const cop_lpm_table *tab, int form, uint32_t xbits, const uint32_t *ips, uint32_t n,
                      uint32_t *out, uint32_t *ref, uint32_t *info);

/* ---- live tables (lpm_live.c) ------------------------------------------ */
void cop_lpm_live_free(struct cop_lpm_live *l);
uint64_t cop_lpm_next_uid(void);
/* Build the index behind add / delete / is_rule_present now (it is otherwise
 * built at the first mutation): makes cop_lpm_is_rule_present O(1). */
int cop_lpm_index(cop_lpm_table *t);
/* The report as the table is now: n_distinct, tbl8_used and n_intervals follow
 * every mutation; the other fields keep what cop_lpm_build counted. */
void cop_lpm_report_get(const cop_lpm_table *t, cop_lpm_report *out);

/* Device entry of a form for an interval value / a rule id. */
static inline uint32_t cop_dir_entry(uint32_t ival)
{
    return (ival & COP_IV_HIT) ? (ival & ~0x02000000u) : 0u; /* nh | valid | depth<<26 */
}
static inline uint32_t cop_rule_entry(const cop_lpm_table *t, uint32_t rule)
{
    if (rule == COP_NO_RULE) return 0u;
    return rule | COP_DIR_VALID | (t->rule_nh[rule] ? COP_RV_DROP : 0u);
}

/* One journalled mutation: the prefix whose address range changed. */
enum { COP_CHG_ADD = 0, COP_CHG_SET = 1, COP_CHG_DEL = 2, COP_CHG_DEL_ALL = 3 };
typedef struct {
    uint32_t ip;     /* masked prefix (0 for DEL_ALL) */
    uint32_t id;     /* rule id taken (ADD), kept (SET) or freed (DEL) */
    uint8_t  depth;  /* 0 for DEL_ALL: the whole address space */
    uint8_t  kind;   /* COP_CHG_* */
} cop_lpm_change;
#define COP_LPM_JOURNAL_CAP 65536u
/* The mutations that took the table from generation `since` to now, oldest
 * first (malloc-ed; NULL when there are none). Returns their number, or
 * -ESTALE when `since` has fallen off the journal ("too old": the caller
 * rebuilds from the whole table), -EINVAL, -ENOMEM. `cap` (tests) shrinks
 * the journal: cop_lpm_journal_set_cap drops all but the newest cap entries. */
int cop_lpm_changes_since(const cop_lpm_table *t, uint64_t since, cop_lpm_change **out);
int cop_lpm_journal_set_cap(cop_lpm_table *t, uint32_t cap);

/* A fill record of the patch kernel (cop_patch.hip): entries
 * [first, first + count) of table (0: tbl24, 1: tbl8) become `entry`. */
typedef struct {
    uint32_t table, first, count, entry;
} cop_patch_rec;

/* Host-side book of one device DIR-24-8 image that accepts patches: which
 * /24 blocks own which tbl8 group, the free groups, the capacity in groups
 * and the table generation the image holds. Group numbers of a fresh image
 * are cop_lpm_form_fill_dir24's (address order); after patches they are the
 * image's own. */
typedef struct cop_live_img cop_live_img;
cop_live_img *cop_live_img_create(const cop_lpm_table *t, int form, uint32_t cap_groups);
void cop_live_img_free(cop_live_img *img);
uint64_t cop_live_img_generation(const cop_live_img *img);
uint32_t cop_live_img_groups_used(const cop_live_img *img);
/* The disjoint fill records that bring the image from its generation to the
 * table's (malloc-ed; *n may be 0), and the image's book with them. rep gets
 * n_changes, tbl24_entries, tbl8_entries, groups_taken, groups_released.
 * 0, -ESTALE (journal too old), -ENOSPC (more groups needed than the image
 * has), -ENOMEM. After an error the book is stale: repaint the whole image
 * and create a new book. */
int cop_lpm_patch_records(const cop_lpm_table *t, cop_live_img *img, cop_patch_rec **recs, uint32_t *n,
                          cop_update_report *rep);
/* Host mirror of the patch kernel: apply records to host arrays of cap24 /
 * cap8 entries. -EINVAL (and nothing written) if a record leaves its array. */
int cop_patch_apply_host(uint32_t *tbl24, uint32_t cap24, uint32_t *tbl8, uint32_t cap8, const cop_patch_rec *recs,
                         uint32_t n);
/* tests: the patch kernel alone, on device buffers the caller allocated
 * (16-byte aligned, cap24 / cap8 entries); synchronous */
int cop_debug_patch(cop_ctx *c, void *tbl24_dptr, uint32_t cap24, void *tbl8_dptr, uint32_t cap8,
                    const cop_patch_rec *recs, uint32_t n);

/* ---- whole-image paint (lpm_build.c, cop_paint.hip) ----------------------- */
/* /24 blocks one workgroup of the paint kernel owns (COPK_PAINT_CHUNK) */
#define COP_PAINT_CHUNK 4096u
/* What the paint kernel reads for a form's DIR-24-8 image: the unmerged
 * (start, entry) intervals cop_lpm_form_fill_dir24 paints from, and the
 * ascending /24 blocks that hold an interval start past their first address
 * (the extended blocks: ext24[g] owns tbl8 group g, fill_dir24's numbering;
 * *n_ext == cop_lpm_form_n_ext). The three arrays are malloc-ed (ext24 has at
 * least one word). 0, -EINVAL, -ENOMEM. */
int cop_lpm_paint_plan(const cop_lpm_table *t, int form, uint32_t **starts, uint32_t **entries, uint32_t *niv,
                       uint32_t **ext24, uint32_t *n_ext);
/* Host mirror of the paint kernel, chunk by chunk and with a search per entry
 * as the kernel does it: all 2^24 tbl24 entries, tbl8 groups 0 .. n_ext - 1,
 * zeros in groups n_ext .. cap_groups - 1. -EINVAL (and nothing written) for
 * niv == 0, starts[0] != 0 or n_ext > cap_groups. */
int cop_paint_host(const uint32_t *starts, const uint32_t *entries, uint32_t niv, const uint32_t *ext24,
                   uint32_t n_ext, uint32_t *tbl24, uint32_t *tbl8, uint32_t cap_groups);
/* tests: the paint kernel alone, on device buffers the caller allocated
 * (16-byte aligned; tbl24: 2^24 entries, tbl8: cap_groups * 256); synchronous */
int cop_debug_paint(cop_ctx *c, const uint32_t *starts, const uint32_t *entries, uint32_t niv, const uint32_t *ext24,
                    uint32_t n_ext, void *tbl24_dptr, void *tbl8_dptr, uint32_t cap_groups);

/* tests: the route stage's table form a launch would use (COPK_TBL_*: 1 LDS
 * intervals, 2 DIR-24-8, 3 trie, 4 bucketed) */
int cop_debug_route_form(cop_ctx *c);
/* tests: the form cop_lookup_bulk uses for a stage (COP_STAGE_FW or
 * COP_STAGE_LPM) now; the same COPK_TBL_* values, plus 0x10 when it is
 * DIR-24-8 with packed tbl8 groups. -EINVAL, -ENOENT. */
int cop_debug_lookup_form(cop_ctx *c, uint32_t stage);
/* tests: what the context's most recent one-shot launch took after the LDS
 * budget ladder (cop_submit): out[0] the firewall stage's form, out[1] the
 * route stage's (COPK_TBL_*, 0 = stage off), out[2] the dynamic LDS bytes per
 * workgroup. -ENOENT before any launch (a launch refused with -E2BIG is
 * none). cop_debug_pmd_forms: the same of a poll-mode kernel. */
int cop_debug_launch_forms(cop_ctx *c, uint32_t out[3]);
int cop_debug_pmd_forms(const cop_pmd *m, uint32_t out[3]);
/* tests: the rest of that launch's kernel instantiation: out[0] the packet
 * layout (COPK_LAY_*: 0 per-lane slot loads, 1 IMIX, 2 coalesced slots,
 * 3 packed 16- or 12-byte records), out[1] the packets per lane (1, 4 or 8;
 * the tile is 256 times that). -ENOENT as above. */
int cop_debug_launch_plan(cop_ctx *c, uint32_t out[2]);

/* ---- bulk lookups (lpm_lookup.c) ---------------------------------------- */
/* What a lookup word keeps of a device entry whose hit bit is set: an NH
 * entry carries the depth in bits 26..31, a tbl8 entry valid_group in bit 25 */
#define COP_LOOKUP_NH_MASK   0x01FFFFFFu
#define COP_LOOKUP_RULE_MASK 0x05FFFFFFu
/* words per staging slot of cop_lookup_bulk_host / cop_lookup_audit (4 MiB) */
#define COP_LOOKUP_STAGE_WORDS (1u << 20)
/* cop_lookup_audit's probe set: for every start s of the form's intervals, s
 * and s - 1 (s > 0), plus 0xFFFFFFFF; ascending, no repeats, at most 2m + 1
 * (malloc-ed). 0, -EINVAL, -ENOMEM. */
int cop_lpm_audit_probes(const cop_lpm_table *t, int form, uint32_t **ips, uint32_t *n);

/* ---- tx gather (tx_gather.c, cop_tx.hip) --------------------------------- */
/* The argument checks cop_tx_gather, cop_submit_tx and cop_tx_gather_host
 * share (include/cop_gpu.h): n_lists lists per batch, seg != 0 for segmented
 * lists, max_batch 0 for no limit. 0, or -EINVAL with *why (may be NULL) the
 * reason. */
int cop_tx_validate(const cop_batch *batches, const cop_tx_desc *tx, uint32_t nb, uint32_t n_lists, int seg,
                    uint32_t max_batch, const char **why);

/* ---- what the side calls' argument checks share (extents.c) ---------------- */
/* One memory extent [start, end) of a call, and whether the call writes it. */
typedef struct {
    uintptr_t start, end;
    int written;
} cop_extent;
/* appends [p, p + bytes) at v[*k]; a NULL p or no bytes: nothing */
void cop_extent_put(cop_extent *v, uint32_t *k, const void *p, uint64_t bytes, int written);
/* what a list call reads of a batch with packets (at most 6 extents): packets
 * (an IMIX slab: its first 16 bytes), offsets, lens (or NULL), results, lists */
void cop_extent_put_batch(cop_extent *v, uint32_t *k, const cop_batch *b, const uint32_t *lens, uint32_t n_lists,
                          int seg);
/* 1 iff a written extent meets an extent the call reads or, unless
 * outputs_may_meet, another written one. Sorts v. */
int cop_extents_clash(cop_extent *v, uint32_t k, int outputs_may_meet);
/* words of fwd_count a batch of n packets has in that layout */
uint32_t cop_tx_fwd_count_words(uint32_t n, uint32_t n_lists, int seg);
/* a packet start of the batch is not 16-byte aligned (pkts, data_off, stride) */
int cop_batch_misaligned(const cop_batch *b);
/* a batch of a list call: the pointers a batch with packets needs, and the alignment above */
int cop_batch_lists_check(const cop_batch *b, const char **why);

/* ---- sketch (sketch.c, cop_sketch.hip) ------------------------------------- */
/* The argument checks the cop_sketch_* device entry points and the host mirror
 * share (include/cop_gpu.h "Sketch"). 0, or -EINVAL with *why (may be NULL)
 * the reason. */
int cop_sketch_config_check(const cop_sketch_config *cfg, const char **why);
int cop_sketch_update_validate(const cop_batch *batches, uint32_t nb, uint32_t verdict_mask, uint32_t max_batch,
                               const char **why);
int cop_sketch_query_validate(const cop_sketch_config *cfg, const void *counters, const uint32_t *ips, uint32_t n,
                              const uint64_t *out, const char **why);
int cop_sketch_police_validate(const cop_sketch_config *cfg, const void *counters, const cop_batch *batches,
                               const cop_police_desc *pol, uint32_t nb, uint32_t n_lists, int seg,
                               uint32_t max_batch, const char **why);

/* ---- AEAD (aead.c, cop_aead.hip) ------------------------------------------- */
/* The argument checks cop_aead_seal / _open, cop_poly1305_bulk and the host
 * mirror share (include/cop_gpu.h "AEAD"): mode one of the three below, otk
 * cop_poly1305_bulk's keys (NULL otherwise), max_batch 0 for no limit on
 * n_frames. 0, or -EINVAL / -ENOMEM with *why (may be NULL) the reason. */
#define COP_AEAD_MODE_SEAL 0
#define COP_AEAD_MODE_OPEN 1
#define COP_AEAD_MODE_POLY 2
int cop_aead_validate(const cop_aead_key *key, const cop_aead_burst *bursts, uint32_t nb, int mode, const uint8_t *otk,
                      uint32_t max_batch, const char **why);

/* ---- L3 forward (fwd.c, cop_fwd.hip) ---------------------------------------- */
/* The argument checks cop_fwd_check / cop_fwd_rewrite and the host mirror
 * share (include/cop_gpu.h "L3 forward"): entries the table (device or host,
 * only its extent is used), max_batch 0 for no limit on n. 0, or -EINVAL /
 * -ENOMEM with *why (may be NULL) the reason. */
int cop_fwd_check_validate(const void *entries, uint32_t n_entries, const cop_fwd_config *cfg, const cop_batch *batches,
                           const cop_fwd_check_desc *desc, uint32_t nb, uint32_t n_lists, int seg, uint32_t max_batch,
                           const char **why);
int cop_fwd_rewrite_validate(const void *entries, uint32_t n_entries, const cop_fwd_config *cfg,
                             const cop_batch *batches, const cop_tx_desc *tx, const cop_fwd_rw_desc *rw, uint32_t nb,
                             uint32_t n_lists, int seg, uint32_t max_batch, const char **why);

/* ---- ACL (acl.c, cop_acl.hip) ------------------------------------------------ */
/* Where the parts of a built image lie, in u32 words from its start (acl.c's
 * head comment; every offset is a multiple of 4): per range field (src, dst,
 * sport, dport) niv starts and niv rows of row_words, the 256 protocol rows,
 * the rank -> word table. */
typedef struct cop_acl_layout {
    uint32_t n_rules, row_words;
    uint32_t niv[4], off_starts[4], off_rows[4];
    uint32_t off_proto, off_rank;
    uint32_t words;   /* the whole image */
    uint32_t _pad;
} cop_acl_layout;
struct cop_acl_table {
    cop_acl_layout lay;
    uint32_t *image;
};
/* The argument checks cop_acl_classify / cop_acl_filter and the host mirror
 * share (include/cop_gpu.h "ACL"): image and counters (or NULL) device or
 * host, only their extents are used; filter != 0 for the filter, whose list
 * layout n_lists / seg is; max_batch 0 for no limit on n. 0, or -EINVAL /
 * -ENOMEM with *why (may be NULL) the reason. */
int cop_acl_validate(const void *image, uint64_t image_bytes, const void *counters, uint32_t n_rules,
                     const cop_batch *batches, const cop_acl_desc *descs, uint32_t nb, int filter, uint32_t n_lists,
                     int seg, uint32_t max_batch, const char **why);

/* Host paths with an explicit stage mask instead of the context's: the
 * drop-in coprocessor API (dropin.c) runs the coprocessor thread's NF chain,
 * COP_DROPIN_STAGES (process_packet, coprocessor.c:50-65). */
int cop_process_host_stages(cop_ctx *c, uint32_t stages, const void *const *pkt_data, uint32_t n,
                            cop_result *results, uint32_t *fwd_idx, uint32_t *fwd_count);
/* cop_config.max_batch of a context (0 for NULL). */
uint32_t cop_ctx_max_batch(const cop_ctx *c);
int cop_host_batch_submit_stages(cop_ctx *c, uint32_t stages, uint32_t slot, const void *const *pkt_data,
                                 uint32_t n);

/* cop_pmd_start_rings with an explicit stage mask (the drop-in's NF chain) */
typedef struct cop_pmd cop_pmd;
int cop_pmd_start_rings_stages(cop_ctx *c, const cop_batch_ring *rings, uint32_t n_rings, uint32_t flags,
                               uint32_t stages, cop_pmd **out);

/* Diagnostics ($COP_HOST_PROF=1): host ns per op of the host batch paths of
 * a context: [0] gather, [1] launch, [2] wait, [3] copy-out, [4] batches,
 * [5] packets; and of the calling thread's drop-in ring loop:
 * [0] drain, [1] batch call, [2] async wait, [3] forward/free, [4] calls,
 * [5] calls with packets, [6] packets. Return the word count. */
int cop_debug_host_prof(cop_ctx *c, uint64_t *out, uint32_t n, int reset);
int cop_debug_dropin_prof(uint64_t *out, uint32_t n, int reset);

#ifdef __cplusplus
}
#endif
#endif
